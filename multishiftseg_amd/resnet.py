"""The ResNet-50 backbone of the Mask2Former configuration, forward only.

Host-side mirror of detectron2's ``build_resnet_backbone`` as ``Base-Cityscapes-SemanticSegmentation.yaml`` configures it
(depth 50, ``STRIDE_IN_1X1: False``, ``res2..res5``, ``NORM: "SyncBN"``) and as ``MaskFormer.forward`` calls it
(lib/network/mask2former/maskformer_model.py:233). detectron2 is not a dependency; the module and parameter names are
detectron2's, so its checkpoints load:

  stem.conv1                 7x7, stride 2, padding 3, no bias, ``.norm``
  res2 .. res5               nn.Sequential of 3 / 4 / 6 / 3 bottleneck blocks
  resK.i.conv1 / conv2 / conv3   1x1 / 3x3 (padding 1, carries the block's stride) / 1x1, no bias, each with ``.norm``
  resK.0.shortcut            1x1 with the block's stride, ``.norm``

``.norm`` is an nn.BatchNorm2d (eps 1e-5): the state-dict keys of the reference's SyncBatchNorm; a FrozenBatchNorm2d checkpoint
(no ``num_batches_tracked``) loads too. The trainer keeps the backbone in eval mode for the whole run (train_m2f.py:409-412), so
every norm is ONE folded affine (mss_bn_fold_eval_f32) in the epilogue of the convolution in front of it.

What runs (all in libmss_hip.so, NHWC inside, NCHW at the boundary as MSDeformAttnPixelDecoder.forward_features takes it):
  * stem: kernels.stem7_conv (csrc/stem7.hip) with the folded norm and the ReLU, then kernels.maxpool3s2;
  * per block three or four kernels.conv2d calls, the norm as ``out_affine``, the ReLU as ``out_relu``; conv3 takes ``res=`` the
    shortcut and the final ReLU. The 3x3 layers take the direct implicit-GEMM route.

Training (stage 2 fine-tunes the whole model, the backbone at 0.1 x lr with its norms in eval mode): opt-in, as the GMA
decoder's. ``ResNet.set_trainable()`` with grad mode enabled runs the SAME forward calls inside one autograd node (_BackboneFn: the
image and the res2..res5 parameters that require a gradient in, the requested NCHW maps out -- bit-identical to the frozen path) and
keeps ``a1``, ``a2`` and ``out`` of every block from the first trainable block on. Its backward walks the blocks in reverse:
  * dz3 = g_out * [out > 0] (the eval-mode form of kernels.bn_relu_backward: unit scale, zero shift);
  * per convolution G = kernels.conv2d_wgrad(input, dz); dW = s * G with s = gamma * rstd the folded norm scale,
    dbeta = sum_pixels dz (kernels.colsum), dgamma = rstd * (<W, G> - running_mean * dbeta) -- the pre-norm output is linear in W, so
    it is neither stored nor recomputed and nothing is divided by gamma (float64 on the device for the small reductions);
  * data gradients: the forward kernels on flip-packed weights with s as the PROLOGUE scale (the flipped pack depends on the weight
    alone), gated by the stored activation through ``res_mask`` (a2 after conv3, a1 after conv2), summed at the block input through
    ``res=``; conv2 and shortcut of res3.0 / res4.0 / res5.0 run kernels.conv2d_dgrad_s2 (csrc/conv_dgrad_s2.hip);
  * only what the ``requires_grad`` pattern asks for; nothing in front of the first trainable block;
  * the stem weight, a second opt-in (``set_trainable(stem=True)``; a plain ``set_trainable()`` still refuses a trainable stem): the
    stem output ``a0`` stays on the tape, the tape starts at res2.0, which is asked for its input gradient g at the pooled map, and the
    walk ends with G = kernels.stem7_wgrad(image, g, a0) (csrc/stem7_wgrad.hip: the max-pool backward, its arg-max recomputed from a0,
    and the ReLU gate run in the kernel's operand loader) and dW = s * G. The stem norm's weight and bias are never trained: the
    reference's FrozenBatchNorm keeps them as buffers, and their dbeta would need dz materialised.
Not built: train-mode BatchNorm; a gradient for the image; gradients of the stem norm's affine. Without set_trainable() a
backbone with trainable parameters raises under grad mode, as before.
"""
import torch
from torch import nn

from . import kernels as K
from .msdeformattn_decoder import ShapeSpec, _NormConv2d


def _conv(cin, cout, k, stride=1, padding=0):
    conv = _NormConv2d(cin, cout, kernel_size=k, stride=stride, padding=padding, bias=False, norm=nn.BatchNorm2d(cout, eps=1e-5))
    nn.init.kaiming_normal_(conv.weight, mode="fan_out", nonlinearity="relu")          # fvcore c2_msra_fill
    return conv


def _folded(conv):
    """The folded eval-mode norm of `conv` as (scale, shift), re-made whenever one of the norm's parameters or running buffers is
    modified in place or moved -- the stale-weight guard of kernels._cached_pack, over all four tensors."""
    bn = conv.norm
    key = tuple((t._version, t.data_ptr()) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
    ent = bn.__dict__.get("_mss_folded")                      # lives on the norm itself and dies with it, as the packed weights do
    if ent is None or ent[0] != key:
        st = K.bn_fold(bn)
        ent = bn.__dict__["_mss_folded"] = (key, (st.scale, st.shift))
    return ent[1]


class BasicStem(nn.Module):
    def __init__(self, in_channels=3, out_channels=64):
        super().__init__()
        self.conv1 = _conv(in_channels, out_channels, 7, stride=2, padding=3)
        self.out_channels, self.stride = out_channels, 4


class BottleneckBlock(nn.Module):
    def __init__(self, in_channels, out_channels, *, bottleneck_channels, stride=1):
        super().__init__()
        self.in_channels, self.out_channels, self.stride = in_channels, out_channels, stride
        self.shortcut = _conv(in_channels, out_channels, 1, stride=stride) if in_channels != out_channels else None
        self.conv1 = _conv(in_channels, bottleneck_channels, 1)                        # STRIDE_IN_1X1 False: the 3x3 strides
        self.conv2 = _conv(bottleneck_channels, bottleneck_channels, 3, stride=stride, padding=1)
        self.conv3 = _conv(bottleneck_channels, out_channels, 1)

    def forward_act(self, x):
        """relu(norm3(conv3(relu(norm2(conv2(relu(norm1(conv1(x)))))))) + shortcut(x)) on an NHWC Act, eval-mode norms."""
        s = self.stride
        sc = x if self.shortcut is None else K.conv2d(x, K.packed(self.shortcut.weight), stride=s, out_affine=_folded(self.shortcut))
        y = K.conv2d(x, K.packed(self.conv1.weight), out_affine=_folded(self.conv1), out_relu=True)
        y = K.conv2d(y, K.packed(self.conv2.weight), stride=s, pad=1, out_affine=_folded(self.conv2), out_relu=True)
        return K.conv2d(y, K.packed(self.conv3.weight), out_affine=_folded(self.conv3), out_relu=True, res=sc)

    def forward_act_saving(self, x, tape):
        """forward_act through the same calls; (block, x, a1, a2, out) goes onto `tape` for backward_act."""
        s = self.stride
        sc = x if self.shortcut is None else K.conv2d(x, K.packed(self.shortcut.weight), stride=s, out_affine=_folded(self.shortcut))
        a1 = K.conv2d(x, K.packed(self.conv1.weight), out_affine=_folded(self.conv1), out_relu=True)
        a2 = K.conv2d(a1, K.packed(self.conv2.weight), stride=s, pad=1, out_affine=_folded(self.conv2), out_relu=True)
        out = K.conv2d(a2, K.packed(self.conv3.weight), out_affine=_folded(self.conv3), out_relu=True, res=sc)
        tape.append((self, x, a1, a2, out))
        return out

    def backward_act(self, g, x, a1, a2, out, need_dx, grads):
        """g: gradient at the block's output (Act). Fills `grads` (parameter -> gradient) for this block's parameters that require
        one and returns the gradient at the block's input (Act), or None without need_dx. Formulas: the module docstring."""
        s = self.stride
        dz3 = _relu_gate(g, out)
        _param_grads(self.conv3, a2, dz3, 1, 0, grads)
        if self.shortcut is not None:
            _param_grads(self.shortcut, x, dz3, s, 0, grads)
        below = need_dx or _wants(self.conv1)
        if not (below or _wants(self.conv2)):
            return None
        dz2 = _dgrad(self.conv3, dz3, 1, None, res=a2, res_mask=True)
        _param_grads(self.conv2, a1, dz2, s, 1, grads)
        if not below:
            return None
        dz1 = _dgrad(self.conv2, dz2, s, (a1.H, a1.W), res=a1, res_mask=True)
        _param_grads(self.conv1, x, dz1, 1, 0, grads)
        if not need_dx:
            return None
        through = dz3 if self.shortcut is None else _dgrad(self.shortcut, dz3, s, (x.H, x.W))
        return _dgrad(self.conv1, dz1, 1, None, res=through)


def _wants(conv):
    return conv.weight.requires_grad or conv.norm.weight.requires_grad or conv.norm.bias.requires_grad


def _relu_gate(g, out):
    """g * [out > 0]: the backward of the block's last ReLU from its stored OUTPUT -- kernels.bn_relu_backward in eval mode with unit
    scale and zero shift."""
    st = K.BNState()
    dev = out.buf.device
    st.scale, st.shift, st.train = K.ones(out.C, dev), K.zeros(out.C, dev), False
    st.save_mean = st.save_invstd = None
    return K.bn_relu_backward(g, out, st)[0]


def _dgrad(conv, dz, stride, out_hw, res=None, res_mask=False):
    """Data gradient of norm(conv(.)) at dz: the forward kernel (stride 1) or kernels.conv2d_dgrad_s2 (stride 2) on the flip-packed
    weight, the folded norm scale as the prologue scale of dz; `res` added, or gating with res_mask."""
    pw = K.packed(conv.weight, flip=True)
    aff = (_folded(conv)[0], K.zeros(conv.weight.shape[0], conv.weight.device))
    if stride == 2:
        return K.conv2d_dgrad_s2(dz, pw, out_hw, in_affine=aff, res=res, res_mask=res_mask)
    return K.conv2d(dz, pw, pad=conv.weight.shape[2] // 2, in_affine=aff, res=res, res_mask=res_mask)


def _param_grads(conv, x, dz, stride, pad, grads):
    """dW = s * G, dbeta = sum dz, dgamma = rstd * (<W, G> - running_mean * dbeta) of y = norm(conv(x)), G = wgrad(x, dz); each only
    where the parameter requires a gradient. The per-channel reductions and the subtraction run in float64 on the device."""
    bn = conv.norm
    need_w, need_g, need_b = conv.weight.requires_grad, bn.weight.requires_grad, bn.bias.requires_grad
    if not (need_w or need_g or need_b):
        return
    if need_w or need_g:
        k, c, r, _ = conv.weight.shape
        G = K.conv2d_wgrad(x, dz, k, c, r, r, stride=stride, pad=pad)
    if need_w:
        grads[conv.weight] = G * _folded(conv)[0].view(-1, 1, 1, 1)
    if need_g or need_b:
        dbeta = K.colsum(dz).double().sum(0)
    if need_b:
        grads[bn.bias] = dbeta.float()
    if need_g:
        rstd = (bn.running_var.double() + bn.eps).rsqrt()
        wg = (conv.weight.detach().double() * G.double()).sum((1, 2, 3))
        grads[bn.weight] = (rstd * (wg - bn.running_mean.double() * dbeta)).float()


class _BackboneFn(torch.autograd.Function):
    """image, the parameters that require a gradient (the stem weight first, where it is trained; then those of res2..res5) -> the
    requested NCHW maps. The Acts between the blocks never become tensors; the tape holds (block, x, a1, a2, out) from the first
    trainable block on -- from res2.0 on with a trainable stem, whose output a0 is kept beside it."""

    @staticmethod
    def forward(ctx, model, x, *params):
        tape, stem = [], {}
        out = model._run(x, tape, params, stem)
        ctx.model, ctx.tape, ctx.params = model, tape, params
        ctx.stem = (x.detach(), stem["a0"]) if stem else None
        ctx.ends = [id(getattr(model, n)[-1]) for n in out]          # the block whose `out` each returned map is
        return tuple(out.values())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *gouts):
        tape, grads = ctx.tape, {}
        entering = {end: g for end, g in zip(ctx.ends, gouts) if g is not None}
        g = None
        for i in range(len(tape) - 1, -1, -1):
            blk, x, a1, a2, out = tape[i]
            tape[i] = None                                           # the stored activations go as the walk passes them
            gin = entering.get(id(blk))
            if gin is not None:                                      # a returned map: its gradient joins the next stage's data gradient
                if g is None:
                    g = K.Act.empty(out.N, out.H, out.W, out.C, out.buf.device)
                    K.nchw_into_rows(gin, g.ptr, g.ld, g.H * g.W * g.ld)
                else:
                    K.nchw_into_rows(gin, g.ptr, g.ld, g.H * g.W * g.ld, accumulate=True)
            if g is None:
                continue
            g = blk.backward_act(g, x, a1, a2, out, i > 0 or ctx.stem is not None, grads)
        if ctx.stem is not None and g is not None:                   # g: the gradient at the pooled map, res2.0's input
            img, a0 = ctx.stem
            conv1 = ctx.model.stem.conv1
            grads[conv1.weight] = K.stem7_wgrad(img.float(), g, a0) * _folded(conv1)[0].view(-1, 1, 1, 1)
        ctx.tape = ctx.stem = None
        return (None, None) + tuple(grads.get(p) for p in ctx.params)


def _load_without_counters(module, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
    """A FrozenBatchNorm2d checkpoint has no num_batches_tracked: keep the module's own counter instead of reporting it missing."""
    for name, m in module.named_modules():
        if isinstance(m, nn.BatchNorm2d) and m.num_batches_tracked is not None:
            key = f"{prefix}{name}.num_batches_tracked"
            if key not in state_dict:
                state_dict[key] = m.num_batches_tracked.detach().clone()


class ResNet(nn.Module):
    size_divisibility = 32

    def __init__(self, stem, stages, out_features):
        super().__init__()
        self.stem = stem
        self.stage_names = []
        self._out_feature_channels, self._out_feature_strides = {}, {}
        stride = stem.stride
        for i, blocks in enumerate(stages):
            name = f"res{i + 2}"
            self.add_module(name, nn.Sequential(*blocks))
            self.stage_names.append(name)
            stride *= blocks[0].stride
            self._out_feature_channels[name], self._out_feature_strides[name] = blocks[-1].out_channels, stride
        bad = [f for f in out_features if f not in self.stage_names]
        if bad:
            raise NotImplementedError(f"ResNet (multishiftseg_amd): out_features among {self.stage_names}, got {bad}")
        self._out_features = list(out_features)
        self._trainable = self._train_stem = False
        self.register_load_state_dict_pre_hook(_load_without_counters)

    def set_trainable(self, flag=True, stem=False):
        """Opt in to (or out of) the differentiable path: with the switch on, in eval mode and with grad mode enabled, forward() runs
        as one autograd node over the same kernels and the res2..res5 parameters that require a gradient receive one. Off (the
        default) the backbone is forward-only, as before; under torch.no_grad() the switch makes no difference.

        stem=True (a second opt-in; without it a trainable stem raises as before): stem.conv1.weight receives a gradient too where
        it requires one (kernels.stem7_wgrad). The stem norm's weight and bias still raise when they require a gradient: the
        reference's FrozenBatchNorm never trains them, and their dbeta would need the stem's dz materialised, which the fused kernel
        never does."""
        self._trainable = bool(flag)
        self._train_stem = bool(flag) and bool(stem)
        return self

    def freeze(self, freeze_at=0, norms=False):
        """detectron2's ResNet.freeze: the stem for freeze_at >= 1, then res2 ... by index (freeze_at >= 2 freezes res2, ...):
        requires_grad=False on the convolution weights AND the norm parameters of the frozen parts. norms=True also freezes the
        norm parameters of every other part. Returns self.

        The reference config (anomaly_ft.yaml: FREEZE_AT 5, NORM "BN") turns every backbone norm into a FrozenBatchNorm2d, whose
        affine is a buffer, and stage 2's trainable_params_name_update ["."] then re-enables the convolution weights only. The
        faithful stage-2 set-up here is therefore ``freeze(0, norms=True)`` with ``set_trainable(stem=True)``: all norm parameters
        frozen, the 53 convolution weights (stem.conv1.weight and the 52 of res2..res5) trainable. ``freeze(1, norms=True)`` (the stem
        weight frozen too, 52 weights) remains valid and needs no stem opt-in. Norm-parameter gradients are built all the same in
        res2..res5, for users who keep the norms' affines as parameters; the stem norm's are not."""
        for idx, part in enumerate([self.stem] + [getattr(self, n) for n in self.stage_names], start=1):
            if freeze_at >= idx:
                for p in part.parameters():
                    p.requires_grad_(False)
        if norms:
            for m in self.modules():
                if isinstance(m, nn.BatchNorm2d):
                    for p in m.parameters():
                        p.requires_grad_(False)
        return self

    def output_shape(self):
        return {n: ShapeSpec(channels=self._out_feature_channels[n], stride=self._out_feature_strides[n]) for n in self._out_features}

    def _check_mode(self, x):
        """Raises what is not built; returns the parameters the differentiable path returns gradients for (empty: frozen path)."""
        if self.training:
            raise NotImplementedError("ResNet (multishiftseg_amd): train-mode BatchNorm is not built (the reference keeps the backbone "
                                      "in eval mode, train_m2f.py:409-412); call .eval()")
        if not (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))):
            return ()
        if not self._trainable:
            raise NotImplementedError("ResNet (multishiftseg_amd): no backward (forward only); freeze the backbone's parameters or call "
                                      "under torch.no_grad()")
        if x.requires_grad:
            raise NotImplementedError("ResNet (multishiftseg_amd): no gradient for the image is built (the data gradient stops at the "
                                      "first trainable block); detach the image")
        stem = [n for n, p in self.stem.named_parameters() if p.requires_grad]
        norm = [n for n in stem if n != "conv1.weight"]
        if norm and self._train_stem:
            raise NotImplementedError(f"ResNet (multishiftseg_amd): a trainable stem norm is not built (stem.{norm[0]} requires a "
                                      "gradient: the reference's FrozenBatchNorm never trains it, and its dbeta would need the stem's dz "
                                      "materialised); freeze(0, norms=True) freezes the norms")
        if stem and not self._train_stem:
            raise NotImplementedError(f"ResNet (multishiftseg_amd): a trainable stem is not built (stem.{stem[0]} requires a gradient) "
                                      "without its own opt-in: set_trainable(stem=True) trains stem.conv1.weight (never the stem "
                                      "norm's affine); freeze(1) freezes the stem")
        head = (self.stem.conv1.weight,) if stem else ()
        return head + tuple(p for name in self._run_stages() for p in getattr(self, name).parameters() if p.requires_grad)

    def _run_stages(self):
        """The stages forward() runs: up to the last requested one."""
        last = max(self.stage_names.index(f) for f in self._out_features)
        return self.stage_names[:last + 1]

    def _run(self, x, tape=None, params=(), stem=None):
        """stem -> stages -> {name: NCHW map}. tape (a list): from the first block that owns one of `params` on, every block leaves
        (block, x, a1, a2, out) there -- the same kernel calls either way. stem (a dict): where the stem weight is among `params`
        the stem output goes there as "a0" and the tape starts at res2.0."""
        conv1 = self.stem.conv1
        a0 = K.stem7_conv(x.float(), conv1.weight, _folded(conv1), relu=True)
        y = K.maxpool3s2(a0)
        wanted = {id(p) for p in params}
        from_start = stem is not None and id(conv1.weight) in wanted
        if from_start:
            stem["a0"] = a0
        out = {}
        for name in self._run_stages():
            for blk in getattr(self, name):
                if tape is not None and (tape or from_start or any(id(p) in wanted for p in blk.parameters())):
                    y = blk.forward_act_saving(y, tape)
                else:
                    y = blk.forward_act(y)
            if name in self._out_features:
                out[name] = K.nhwc_to_nchw(y)
        return out

    # ---- reference API ----------------------------------------------------------------------------------------------------
    def forward(self, x):
        params = self._check_mode(x)
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"ResNet takes [N, 3, H, W] images, got {tuple(x.shape)}")
        if not x.is_cuda:
            raise RuntimeError("ResNet (multishiftseg_amd) runs on an MI355X only; there is no CPU path")
        if params:
            maps = _BackboneFn.apply(self, x, *params)
            return dict(zip([n for n in self._run_stages() if n in self._out_features], maps))
        with torch.no_grad():
            return self._run(x)


def build_resnet_backbone(depth=50, out_features=("res2", "res3", "res4", "res5"), stem_out_channels=64, res2_out_channels=256,
                          stride_in_1x1=False):
    """detectron2's build_resnet_backbone for the configuration the reference loads (dilation 1, one group, 64 channels per group)."""
    if depth != 50:
        raise NotImplementedError(f"ResNet (multishiftseg_amd): depth 50 is what the Mask2Former config loads, got {depth}")
    if stride_in_1x1:
        raise NotImplementedError("ResNet (multishiftseg_amd): STRIDE_IN_1X1 True (the MSRA layout) is not built; the config sets False")
    if stem_out_channels != 64:
        raise NotImplementedError(f"ResNet (multishiftseg_amd): the 7x7 stem kernel has 64 output channels, got {stem_out_channels}")
    stem = BasicStem(3, stem_out_channels)
    stages, cin, cout, mid = [], stem_out_channels, res2_out_channels, res2_out_channels // 4
    for idx, nblocks in enumerate((3, 4, 6, 3)):
        blocks = []
        for i in range(nblocks):
            blocks.append(BottleneckBlock(cin, cout, bottleneck_channels=mid, stride=2 if (i == 0 and idx > 0) else 1))
            cin = cout
        stages.append(blocks)
        cout, mid = cout * 2, mid * 2
    return ResNet(stem, stages, out_features)
