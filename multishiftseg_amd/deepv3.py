"""DeepWV3Plus on MI355X: the reference's module contract, executed by hand-written HIP kernels.

Host-side mirror of lib/network/deepv3/deepv3.py:203-285 (DeepWV3Plus, ASPP) and
lib/network/deepv3/wider_resnet.py:64-182,267-364 (WiderResNetA2 trunk): same constructor, same
``forward(inp) -> (anomaly_score [B,H,W], logit [B,num_classes,H,W])`` for 2..100 classes, same parameter / buffer names (the
269 state-dict entries load unchanged), same train()/eval() behaviour of BatchNorm and Dropout2d,
same ``uncertainty_func_init``. The nn.Conv2d / nn.BatchNorm2d children are parameter containers
only -- their forward is never called. What runs instead (all in libmss_hip.so):

  * activations live in NHWC; every conv is the fp32-MFMA implicit GEMM with BatchNorm+ReLU of the
    producer folded into its A-operand load, the residual add folded into its epilogue, Dropout2d
    folded into a per-sample affine, and concats written in place through channel slices;
  * the frozen trunk (mod1..mod7, never trainable in the reference: exps/DeepLab.yaml:10-11) runs
    without autograd; the decoder/heads run inside ONE autograd.Function whose backward is a fixed
    sequence of dgrad/wgrad/BN-backward kernels.
"""
import os
from collections import OrderedDict

import torch
import torch.nn as nn

from . import aspp_plan, kernels as K
from .kernels import Act

_STRUCTURE = [3, 3, 6, 3, 1, 1]
_CHANNELS = [(128, 128), (256, 256), (512, 512), (512, 1024), (512, 1024, 2048), (1024, 2048, 4096)]
_ASPP_RATES = (12, 24, 36)   # output_stride 8 doubles (6, 12, 18): deepv3.py:53-54

# Accuracy-aware Winograd tile caps per trunk module (round 3). F(6x6) rounds 3x coarser than F(4x4), and what a layer's
# rounding does to the logits depends on where the layer sits. Measured at 2x3x1024x2048 in train mode against the
# reference's own outputs (tools/attribute_wino_error.py, profiles/r03/wino_attribution_*.txt): ONE mod2 layer on F(6x6)
# moves the logits by 3-4e-5 rms (max 2.9e-4), one mod3 layer by 2e-5, one mod4 layer by 1-2e-5, a mod5..mod7 / ASPP /
# decoder layer by <= 1.2e-5 -- the residual stream is small early on and every later BatchNorm re-amplifies what was
# injected into it. Contributions add in quadrature, so the cap goes where the error per saved millisecond is largest
# (max |dlogit| against the direct kernels / against the reference, argmax flips of 4.2 M pixels, step time, same box):
#   fast      every layer on the cheapest tile (the round-2 policy)     7.1e-4 / 5.6e-4   691 flips   107.96 ms
#   balanced  mod2 + mod3 on F(4x4)                                       3.3e-4 / 2.7e-4   382         109.34 ms
#   strict    mod2 + mod3 + mod4 on F(4x4)  (DEFAULT)                     2.4e-4 / 1.7e-4   243         109.70 ms
# (the direct kernels themselves: - / 7.7e-5, 118 flips; every layer on F(4x4): 1.6e-4 / 1.3e-4, 184 flips, ~118 ms.)
# mod4 costs next to nothing on F(4x4): its F(6x6) products have 1892 rows = 3.75 rounds of GEMM tiles.
_WINO_CAPS = {"fast": {}, "balanced": {"mod2": 4, "mod3": 4}, "strict": {"mod2": 4, "mod3": 4, "mod4": 4}}


def wino_cap(module_name):
    """Largest Winograd output tile the trunk module `module_name` may use (MSS_WINO_ACCURACY=fast|balanced|strict)."""
    mode = os.environ.get("MSS_WINO_ACCURACY", "strict")
    if mode not in _WINO_CAPS:
        raise ValueError(f"MSS_WINO_ACCURACY={mode!r}: expected one of {sorted(_WINO_CAPS)}")
    return _WINO_CAPS[mode].get(module_name, 6)


def _bnrelu(c):
    return nn.Sequential(nn.BatchNorm2d(c), nn.ReLU(inplace=True))


class _Block(nn.Module):
    """Parameter container with the names of IdentityResidualBlock (wider_resnet.py:64-167)."""

    def __init__(self, cin, channels, stride, dilation, drop_p):
        super().__init__()
        self.stride, self.dilation, self.drop_p = stride, dilation, drop_p
        self.bottleneck = len(channels) == 3
        self.bn1 = _bnrelu(cin)
        if not self.bottleneck:
            layers = [("conv1", nn.Conv2d(cin, channels[0], 3, stride=stride, padding=dilation, bias=False,
                                          dilation=dilation)),
                      ("bn2", _bnrelu(channels[0])),
                      ("conv2", nn.Conv2d(channels[0], channels[1], 3, padding=dilation, bias=False,
                                          dilation=dilation))]
            if drop_p is not None:
                layers.insert(2, ("dropout", nn.Dropout2d(p=drop_p)))
        else:
            layers = [("conv1", nn.Conv2d(cin, channels[0], 1, stride=stride, bias=False)),
                      ("bn2", _bnrelu(channels[0])),
                      ("conv2", nn.Conv2d(channels[0], channels[1], 3, padding=dilation, bias=False,
                                          dilation=dilation)),
                      ("bn3", _bnrelu(channels[1])),
                      ("conv3", nn.Conv2d(channels[1], channels[2], 1, bias=False))]
            if drop_p is not None:
                layers.insert(4, ("dropout", nn.Dropout2d(p=drop_p)))
        self.convs = nn.Sequential(OrderedDict(layers))
        if stride != 1 or cin != channels[-1]:
            self.proj_conv = nn.Conv2d(cin, channels[-1], 1, stride=stride, bias=False)


class _ASPP(nn.Module):
    """Names of _AtrousSpatialPyramidPoolingModule (deepv3.py:47-82)."""

    def __init__(self, in_dim=4096, red=256):
        super().__init__()
        feats = [nn.Sequential(nn.Conv2d(in_dim, red, 1, bias=False), nn.BatchNorm2d(red), nn.ReLU(inplace=True))]
        for r in _ASPP_RATES:
            feats.append(nn.Sequential(nn.Conv2d(in_dim, red, 3, dilation=r, padding=r, bias=False),
                                       nn.BatchNorm2d(red), nn.ReLU(inplace=True)))
        self.features = nn.ModuleList(feats)
        self.img_pooling = nn.AdaptiveAvgPool2d(1)
        self.img_conv = nn.Sequential(nn.Conv2d(in_dim, red, 1, bias=False), nn.BatchNorm2d(red),
                                      nn.ReLU(inplace=True))


class _ComposedWeight:
    """One composed ASPP weight W_d o M as the compose GEMM left it: `rows`, its tap-major rows [R*S][kp][ld] (a view of the one result
    buffer), and the dense [K][C][R][S] tensor, which is unpacked when a consumer first asks for it -- eval, the dense route and
    GraphedEval do; the dropped-channel route reads the rows alone (kernels.aspp_dropped_weights) and never pays for that pass."""
    __slots__ = ("shape", "rows", "ld", "kp", "_dense")

    def __init__(self, shape, rows, ld, kp):
        self.shape, self.rows, self.ld, self.kp, self._dense = torch.Size(shape), rows, ld, kp, None

    def dense(self):
        if self._dense is None:
            k, c, r, s_ = self.shape
            g = torch.empty(tuple(self.shape), device=self.rows.device, dtype=torch.float32)
            K.call("mss_conv2d_unpack_wgrad_f32", K.ptr(self.rows), K.ptr(g), k, c, r, s_, self.kp, self.ld, 0, None, None, 0, 0)
            self._dense = g
        return self._dense

    def made(self):
        """The dense tensor if a consumer has asked for it, else None (what GraphedEval keeps alive)."""
        return self._dense


def _dense(w):
    return w.dense() if isinstance(w, _ComposedWeight) else w


class _HeadFn(torch.autograd.Function):
    """Decoder + heads (deepv3.py:270-283) as one differentiable node."""

    @staticmethod
    def forward(ctx, model, x, m2, size, *params):
        score, logit, saved = model._head_forward(x, m2, size, keep=True)
        ctx.model, ctx.saved = model, saved
        return score, logit

    @staticmethod
    def backward(ctx, dscore, dlogit):
        grads = ctx.model._head_backward(ctx.saved, dscore, dlogit, ctx.needs_input_grad[4:])
        ctx.saved = None
        return (None, None, None, None) + tuple(grads)


MIN_CLASSES, MAX_CLASSES = 2, 100      # class indices above 99 mean "OOD" to RelContrastiveLoss and label_threshold; labels are uint8


def heads_layout(num_classes):
    """Layout of the fused heads GEMM (final.6 and ood_head share their input) -> (q, Kh): final.6 lives in rows [0, C) and
    ood_head in rows [q, q + C) of Kh, q = C rounded up to a channel quad (the 16-byte unit of the OOD-score tail), Kh = 2q
    rounded up to 16; every other row is zero. (20, 48) for the 19 Cityscapes classes."""
    C = int(num_classes)
    if C < 1:
        raise ValueError(f"num_classes must be positive, got {num_classes}")
    q = 4 * ((C + 3) // 4)
    return q, 16 * ((2 * q + 15) // 16)


class DeepWV3Plus(nn.Module):
    """Wide-ResNet-38 DeepLabV3+ with the extra OOD head (deepv3.py:203-285)."""

    def __init__(self, num_classes, criterion=None, trunk="WideResnet38"):
        super().__init__()
        if not MIN_CLASSES <= num_classes <= MAX_CLASSES:
            raise ValueError(f"num_classes must be in {MIN_CLASSES}..{MAX_CLASSES} (the range of the HIP OOD-score tail), "
                             f"got {num_classes}")
        self.mod1 = nn.Sequential(OrderedDict([("conv1", nn.Conv2d(3, 64, 3, stride=1, padding=1, bias=False))]))
        cin = 64
        for mod_id, num in enumerate(_STRUCTURE):
            blocks = []
            for b in range(num):
                dil = 2 if mod_id == 3 else (4 if mod_id > 3 else 1)        # wider_resnet.py:322-332
                stride = 2 if (b == 0 and mod_id == 2) else 1
                drop = 0.3 if mod_id == 4 else (0.5 if mod_id == 5 else None)  # wider_resnet.py:334-339
                blocks.append((f"block{b + 1}", _Block(cin, _CHANNELS[mod_id], stride, dil, drop)))
                cin = _CHANNELS[mod_id][-1]
            setattr(self, f"mod{mod_id + 2}", nn.Sequential(OrderedDict(blocks)))
        self.pool2 = nn.MaxPool2d(3, stride=2, padding=1)
        self.pool3 = nn.MaxPool2d(3, stride=2, padding=1)
        self.aspp = _ASPP(4096, 256)
        self.bot_fine = nn.Conv2d(128, 48, kernel_size=1, bias=False)
        self.bot_aspp = nn.Conv2d(1280, 256, kernel_size=1, bias=False)
        self.final = nn.Sequential(
            nn.Conv2d(256 + 48, 256, kernel_size=3, padding=1, bias=False), nn.BatchNorm2d(256),
            nn.ReLU(inplace=True),
            nn.Conv2d(256, 256, kernel_size=3, padding=1, bias=False), nn.BatchNorm2d(256), nn.ReLU(inplace=True),
            nn.Conv2d(256, num_classes, kernel_size=1, bias=False))
        self.ood_head = nn.Conv2d(256, num_classes, kernel_size=1, bias=False)
        self.criterion = criterion
        self.num_classes = num_classes
        self._heads_cache = None
        self._compose_cache = None         # the ASPP weights composed with the trunk's last 1x1 pair (_aspp_composed)
        # data-parallel hook: callable(name, grad_tensor) invoked inside the backward as soon as a
        # parameter gradient has been produced (multishiftseg_amd/ddp.py launches its all-reduce there)
        self.grad_sink = None
        # test hook: {"mod6": [N,1024], "mod7": [N,2048]} pre-scaled Dropout2d masks
        self.dropout_masks = None
        # eval only: forward returns (anomaly_score, None) and skips the 160 MB upsampled logit volume -- what the
        # reference's test loop consumes (test_deeplab.py:92-96 keeps anomaly_score only)
        self.score_only = False

    # ---- reference API ---------------------------------------------------------------------
    def energy_func(self, logit):
        """-logsumexp over classes (deepv3.py:251-253); the fused kernel computes the same thing."""
        return -(1.0 * torch.logsumexp(logit, dim=1))

    def uncertainty_func_init(self):
        """deepv3.py:255-256."""
        self.ood_head.weight.data = self.final[-1].weight.data.clone()

    # ---- parameter bookkeeping -----------------------------------------------------------------
    def _head_params(self):
        names, params = [], []
        for prefix, mod in (("aspp", self.aspp), ("bot_fine", self.bot_fine), ("bot_aspp", self.bot_aspp),
                            ("final", self.final), ("ood_head", self.ood_head)):
            for n, p in mod.named_parameters():
                names.append(f"{prefix}.{n}")
                params.append(p)
        return names, params

    def _check_trunk_frozen(self):
        for i in range(1, 8):
            for n, p in getattr(self, f"mod{i}").named_parameters():
                if p.requires_grad:
                    raise NotImplementedError(
                        f"mod{i}.{n} requires grad: the WideResNet trunk is frozen in both training stages of the "
                        "reference (exps/DeepLab.yaml:10-11) and has no backward kernels here")

    # ---- trunk ------------------------------------------------------------------------------------
    def _dropout_affine(self, st, blk, name, n, want_mask=False):
        """Dropout2d on relu(bn(x)) == per-sample affine: relu(z)*m = relu(z*m) for m >= 0. want_mask: (affine, mask [n, C] or None)."""
        aff, mask = self._dropout_affine_mask(st, blk, name, n)
        return (aff, mask) if want_mask else aff

    def _dropout_affine_mask(self, st, blk, name, n):
        if blk.drop_p is None or not self.training:
            return (st.scale, st.shift), None
        if self.dropout_masks is not None:
            mask = self.dropout_masks[name].to(st.scale.device, torch.float32)
        else:
            keep = 1.0 - blk.drop_p
            mask = torch.bernoulli(torch.full((n, st.scale.numel()), keep, device=st.scale.device)) / keep
        return ((st.scale[None, :] * mask).contiguous(), (st.shift[None, :] * mask).contiguous()), mask.contiguous()

    def _run_block(self, blk, a, name, out_stats=False, factors=False):
        """out_stats: the block's output kernel leaves its per-64-row column sums even in eval mode (the trunk's last block: the ASPP
        image-pooling branch takes its global average from them, kernels.gap). factors (a bottleneck with proj_conv, the trunk's
        last block on the composed ASPP route): neither proj_conv nor conv3 runs; the answer is the pair of prologue factors whose
        products they would have added, a kernels.FactoredAct."""
        train = self.training
        st1 = K.bn_fold(blk.bn1[0], a, train)
        aff1 = (st1.scale, st1.shift)
        if factors:
            shortcut = None
        elif hasattr(blk, "proj_conv"):
            shortcut = K.conv2d(a, K.packed(blk.proj_conv.weight), stride=blk.stride, in_affine=aff1, in_relu=True)
        else:
            shortcut = a
        d = blk.dilation
        c = blk.convs
        cap = wino_cap(name)
        if not blk.bottleneck:
            # want_stats: the producing kernel leaves the batch statistics the next train-mode BatchNorm needs
            o = K.conv3x3(a, c.conv1.weight, dil=d, stride=blk.stride, in_affine=aff1, in_relu=True, want_stats=train,
                          max_tile=cap)
            st2 = K.bn_fold(c.bn2[0], o, train)
            return K.conv3x3(o, c.conv2.weight, dil=d, in_affine=self._dropout_affine(st2, blk, name, a.N), in_relu=True,
                             res=shortcut, want_stats=train or out_stats, max_tile=cap)
        o = K.conv2d(a, K.packed(c.conv1.weight), stride=blk.stride, in_affine=aff1, in_relu=True, want_stats=train)
        st2 = K.bn_fold(c.bn2[0], o, train)
        o2 = K.conv3x3(o, c.conv2.weight, dil=d, in_affine=(st2.scale, st2.shift), in_relu=True, want_stats=train,
                       max_tile=cap)
        st3 = K.bn_fold(c.bn3[0], o2, train)
        aff3, mask = self._dropout_affine(st3, blk, name, a.N, want_mask=True)
        if factors:
            return K.FactoredAct(a, aff1, o2, aff3, mask)
        pw3 = K.packed(c.conv3.weight)
        if mask is not None and K.dropout_compact_wanted(o2, pw3, aff3, shortcut):
            # the dropped channels are exact zeros behind the prologue: each sample multiplies its kept channels only
            return K.conv2d_dropped(o2, pw3, mask, aff3, res=shortcut, want_stats=train or out_stats)
        return K.conv2d(o2, pw3, in_affine=aff3, in_relu=True, res=shortcut, want_stats=train or out_stats)

    def _run_trunk(self, inp):
        fused_stem = os.environ.get("MSS_STEM_FUSED", "1") != "0"
        if fused_stem:
            # mod1.conv1 + pool2 in one kernel (csrc/stem.hip): image in, pooled 64-channel map out; MSS_STEM_FUSED=0 keeps the
            # two routes below + the separate pool (independent second formulations, compared in the tests)
            a = K.stem_conv_pool(inp, self.mod1.conv1.weight)
        elif os.environ.get("MSS_STEM_IM2COL", "1") != "0":
            # 3 -> 64 stem as a dense K = 27 (32) GEMM on explicit 3x3 patches; MSS_STEM_IM2COL=0: the implicit-GEMM
            # kernel on the image padded to 16 channels (K = 144, 13/16 zeros) -- kept as the independent second route
            a = K.conv2d(K.stem_im2col(inp), K.packed_stem(self.mod1.conv1.weight))
        else:
            a = K.conv2d(K.image_to_nhwc(inp, 16), K.packed(self.mod1.conv1.weight), pad=1)
        m2 = None
        for mod_id in range(6):
            name = f"mod{mod_id + 2}"
            if mod_id < 2 and not (fused_stem and mod_id == 0):
                a = K.maxpool3s2(a)
            blocks = list(getattr(self, name))
            for i, blk in enumerate(blocks):
                last = mod_id == 5 and i == len(blocks) - 1
                a = self._run_block(blk, a, name, out_stats=last, factors=last and self._aspp_compose_gate(blk, a))
            if mod_id == 0:
                m2 = a
        return a, m2

    # ---- ASPP composed with the trunk's last 1x1 pair ---------------------------------------------------------------------
    # The trunk output x = Wproj . u + W3 . v (u = relu(bn1(a7)), v = dropout(relu(bn3(o2)))) meets no BatchNorm or nonlinearity
    # before ASPP, and ASPP's four convolutions and its global average are linear in x. With M = [Wproj | W3] ([4096][2048 + 2048],
    # frozen) and w = [u ; v]: conv_d(x; W_d) = conv_d(w; W_d o M) exactly (a bias-free 1x1 maps zero padding to zero padding),
    # GAP(x) = M . GAP(w), dW_d = (dY (x) w) . M^T. The two 2048 -> 4096 products over every pixel become weight-sized products:
    # one compose GEMM (7168 tap-major weight rows x 4096 x 4096) whenever an ASPP weight has changed, one projection of the four
    # weight gradients through M in the backward (DESIGN: "ASPP composed with mod7's output convolutions").
    def _aspp_compose_gate(self, blk, a):
        """True where the trunk's last block hands ASPP its factors: aspp_plan.compose_wanted, a stride-1 bottleneck with
        proj_conv, and the shapes / policy kernels.aspp_tiles takes (Winograd tiles 4 or 6 on all three rates, no tile hook).
        Everything else -- the direct and F(2x2) routes, small sub-grids -- keeps the present path."""
        if not (K.aspp_compose_wanted() and blk.bottleneck and hasattr(blk, "proj_conv") and blk.stride == 1):
            return False
        feats = self.aspp.features
        c_out = blk.proj_conv.weight.shape[0]
        if blk.convs.conv3.weight.shape[0] != c_out or feats[0][0].weight.shape[1] != c_out \
                or self.aspp.img_conv[0].weight.shape[1] != c_out or a.C != blk.proj_conv.weight.shape[1]:
            return False
        return K.aspp_tiles(a.H, a.W, c_out, _ASPP_RATES, [feats[i][0].weight for i in (1, 2, 3)]) is not None

    def _aspp_rows(self, tensors, pw, dropped=None):
        """The four ASPP-shaped tensors [K][C][R][S] packed tap-major ([R*S][Kpad][C] each, 7168 rows of C in all) and one 1x1 product
        of the rows with `pw`: one _ComposedWeight per tensor, whose rows are views of the one result buffer and whose dense() is the
        result in the tensor's own layout. A five-dimensional tensor is a weight gradient of the dropped-channel products
        ([N][K][C][3][3] in per-image compacted columns, kernels.conv3x3_wgrad_dropped): its pack gathers the columns back to their
        channels and adds the images (`dropped`: that step's kernels.AsppDropped)."""
        dev = tensors[0].device
        C = tensors[0].shape[-3]
        geo = [(t.shape[-4], t.shape[-2], t.shape[-1], K._lib.value("mss_conv2d_kpad", t.shape[-4])) for t in tensors]
        rows = [r * s_ * kp for _, r, s_, kp in geo]
        src = Act.empty(1, 1, sum(rows), C, dev)
        r0 = 0
        for t, (k, r, s_, kp), n in zip(tensors, geo, rows):
            if t.dim() == 5:
                K.call("mss_conv2d_pack_weights_f32", K.ptr(t.detach().contiguous()), K.ptr(src.buf[0, 0, r0:r0 + n]), k, C, r, s_, kp, C, 0,
                       K.ptr(dropped.col), t.shape[0], dropped.C0)
            else:
                K.call("mss_conv2d_pack_weights_f32", K.ptr(t.detach().contiguous()), K.ptr(src.buf[0, 0, r0:r0 + n]), k, C, r, s_, kp, C, 0,
                       None, 0, 0)
            r0 += n
        dst = K.conv2d(src, pw)
        out, r0 = [], 0
        for (k, r, s_, kp), n in zip(geo, rows):
            out.append(_ComposedWeight((k, pw.K, r, s_), dst.buf[0, 0, r0:r0 + n], dst.ld, kp))
            r0 += n
        return out

    def _aspp_composed(self, blk):
        """The composed ASPP weights W_d o M ([256, 4096, 1, 1] as its two K-halves, three [256, 4096, 3, 3] as _ComposedWeight: rows now,
        the dense tensor on first use) and the packed M / M^T.
        M is packed once (the trunk is frozen); the composition is redone when an ASPP weight or a trunk factor has changed
        ((version, data_ptr), as _heads_weight): every step in stage 2, once in stage 1 and in eval."""
        wp, w3 = blk.proj_conv.weight, blk.convs.conv3.weight
        ws = [self.aspp.features[i][0].weight for i in range(4)]
        mkey = tuple((t._version, t.data_ptr()) for t in (wp, w3))
        cc = self._compose_cache
        if cc is None or cc["mkey"] != mkey:
            m = torch.cat([wp.detach(), w3.detach()], dim=1).contiguous()                       # M [4096][2048 + 2048][1][1]
            cc = self._compose_cache = dict(mkey=mkey, M=K.pack_weight(m), Mt=K.pack_weight(m.transpose(0, 1).contiguous()),
                                            c0=wp.shape[1], wkey=None)
        wkey = tuple((t._version, t.data_ptr()) for t in ws)
        if cc["wkey"] != wkey:
            with K._Timed("aspp_compose", 2.0 * sum(t.numel() for t in ws) * cc["Mt"].K, ("compose", len(ws))):
                wc = self._aspp_rows(ws, cc["Mt"])
                w0 = wc[0].dense()                 # the 1x1 branch is always read as its two packed K-halves
            c0 = cc["c0"]
            cc.update(wkey=wkey, wc=wc, rows=[(w.rows, w.ld, w.kp) for w in wc], half0=K.pack_weight(w0[:, :c0].contiguous()),
                      half1=K.pack_weight(w0[:, c0:].contiguous()))
        return cc

    # ---- decoder + heads -------------------------------------------------------------------------
    def _heads_weight(self):
        """final.6 and ood_head share their input: one GEMM over the rows of heads_layout (K = 48, rows 0-18 / 20-38, at 19 classes)."""
        w1, w2 = self.final[6].weight, self.ood_head.weight
        key = (w1._version, w1.data_ptr(), w2._version, w2.data_ptr())
        if self._heads_cache is None or self._heads_cache[0] != key:
            C = self.num_classes
            q, Kh = heads_layout(C)
            wh = torch.zeros((Kh, 256, 1, 1), device=w1.device, dtype=torch.float32)
            wh[0:C] = w1.detach()
            wh[q:q + C] = w2.detach()
            self._heads_cache = (key, K.pack_weight(wh), K.pack_weight(wh, flip=True))
        return self._heads_cache[1], self._heads_cache[2]

    def _head_forward(self, x, m2, size, keep=False, want_logit=True, want_label=False):
        train = self.training
        N, h8, w8 = x.N, x.H, x.W
        h2, w2 = m2.H, m2.W
        dev = x.buf.device
        asp = self.aspp
        if train and N == 1:
            raise ValueError("Expected more than 1 value per channel when training, got input size "
                             f"torch.Size([1, 256, 1, 1])")  # what F.batch_norm raises for aspp.img_conv.1
        raw = Act.empty(N, h8, w8, 1280, dev)                      # concat [img, 1x1, d12, d24, d36], pre-BN
        scale = torch.empty(1280, device=dev)
        shift = torch.empty(1280, device=dev)
        states = []
        aspp_xt = {}
        # the composed route (x a kernels.FactoredAct, _aspp_composed): the branches below run on w = [u ; v] with composed weights
        comp = self._aspp_composed(self.mod7[-1]) if isinstance(x, K.FactoredAct) else None
        fx = x if comp is not None else None
        wts = comp["wc"] if comp is not None else [f[0].weight for f in asp.features]
        # every route decision of the block, taken once (aspp_plan.AsppPlan); what follows executes it
        plan = K.aspp_plan_for(x, _ASPP_RATES, wts[1:], keep, [f[0].weight.requires_grad for f in asp.features[1:]])
        # train mode: the Dropout2d-zeroed channels of v are exact zeros in all three products -- each image multiplies its kept
        # channels only
        drop = K.AsppDropped(fx) if plan.dropped else None
        # the three dilated branches read the same 1 GB map: ONE kernel makes all three Winograd-domain inputs from a single read,
        # on the composed route from the two factors, which also leaves GAP(w); GAP(x) = M . GAP(w)
        pre = gap_w = None
        if plan.dropped_separate:
            pre, gap_w = K.aspp_dropped_separate_transforms(fx, _ASPP_RATES, plan, drop)
        elif plan.single_read or plan.gap_from_kernel:
            pre, gap_w = K.aspp_transforms(x, _ASPP_RATES, plan, drop)
        if plan.materialise:
            x = fx.materialise()
        if comp is None:
            pooled = K.gap(x)
        else:
            if gap_w is None:
                gap_w = K.gap(x)
            pooled = K.conv2d(Act(gap_w.view(N, 1, 1, 4096)), comp["M"]).buf.view(N, 4096)
        # image-pooling branch (deepv3.py:84-88): GAP -> 1x1 -> BN over the N samples -> broadcast
        pooled_act = Act(pooled.view(N, 1, 1, 4096))
        u0 = K.conv2d(pooled_act, K.packed(asp.img_conv[0].weight))
        u0_rows = u0.buf.view(N, 256)
        # every branch's folded BatchNorm goes straight into its 256-channel slice of the concat's (scale, shift) vectors
        st = K.bn_fold(asp.img_conv[1], train=train, x_rows=u0_rows, out=(scale[0:256], shift[0:256]))
        K.broadcast_rows(u0_rows, raw.slice(0, 256))
        states.append(st)
        for i, feat in enumerate(asp.features):
            rate = 1 if i == 0 else _ASPP_RATES[i - 1]
            sl = raw.slice(256 * (i + 1), 256)
            if i == 0 and comp is not None:
                # two K-halves with the factors' own prologues, the second accumulating on the first
                half = K.conv2d(fx.a0, comp["half0"], in_affine=fx.aff0, in_relu=True)
                K.conv2d(fx.a1, comp["half1"], in_affine=fx.aff1, in_relu=True, res=half, out=sl, want_stats=train)
                del half
            elif i == 0:
                K.conv2d(x, K.packed(feat[0].weight), out=sl, want_stats=train)
            elif plan.pair_tile and i in (1, 2):
                if i == 1:
                    sl2 = raw.slice(256 * 3, 256)          # ONE object: conv3x3_pair leaves the batch statistics on it
                    K.conv3x3_pair(x, _dense(wts[1]), _dense(wts[2]), _ASPP_RATES[0], _ASPP_RATES[1], sl,
                                   sl2, plan.pair_tile, want_stats=train, xt=pre.take_pair() if pre else None)
                    pair_slices = {1: sl, 2: sl2}
                sl = pair_slices[i]              # carries the statistics the producing transform left (train-mode BatchNorm)
            else:
                # keep the Winograd-domain input X' for this layer's weight gradient when the three of them fit
                # comfortably (2.25-4x the 4096-channel map each: 10.6 GB in all at 2x1024x2048)
                kx = {} if plan.keep_xt[i - 1] else None
                xt = pre.take(i - 1) if pre else None       # the layer owns it now (kept for the weight gradient, or freed)
                if plan.dropped:
                    rows, ld, kp = comp["rows"][i]
                    ww = K.aspp_dropped_weights(rows, wts[i].shape[0], wts[i].shape[1], kp, ld, plan.tiles[i - 1], drop)
                    K.conv3x3_dropped(x, ww, rate, sl, kx, train, xt, drop)
                    del ww
                else:
                    K.conv3x3(x, _dense(wts[i]), dil=rate, out=sl, keep_xt=kx, want_stats=train, xt=xt)
                del xt
                if kx:
                    aspp_xt[i] = kx["xt"]
            states.append(K.bn_fold(feat[1], sl, train, out=(scale[256 * (i + 1):256 * (i + 2)], shift[256 * (i + 1):256 * (i + 2)])))
        up_small = K.conv2d(raw, K.packed(self.bot_aspp.weight), in_affine=(scale, shift), in_relu=True)
        # dec0 = concat [bot_fine(m2), up(bot_aspp)]: when nothing needs it as a tensor (final.0 is not trained in either stage of
        # exps/DeepLab.yaml, so no weight gradient reads it), the x4 bilinear upsample is interpolated inside final.0's Winograd
        # input transform and the 1 GB map is never stored (kernels.conv3x3_on_upsampled_concat)
        dec0 = f0 = None
        if not (keep and self.final[0].weight.requires_grad):
            f0 = K.conv3x3_on_upsampled_concat(K.conv2d(m2, K.packed(self.bot_fine.weight)), up_small, self.final[0].weight,
                                               want_stats=train)
        if f0 is None:
            dec0 = Act.empty(N, h2, w2, 304, dev)
            K.upsample_ac(up_small, h2, w2, out=dec0.slice(48, 256))
            K.conv2d(m2, K.packed(self.bot_fine.weight), out=dec0.slice(0, 48))
        # the two decoder convolutions keep their Winograd-domain inputs for the weight gradient too (2.3 + 1.9 GB at
        # 2x1024x2048; re-transforming costs 0.73 ms each), under the same budget as the ASPP layers
        dec_xt_bytes = K.wino_xt_bytes(N, h2, w2, 304, 1) + K.wino_xt_bytes(N, h2, w2, 256, 1)
        keep_dec = keep and plan.xt_bytes + dec_xt_bytes < aspp_plan.XT_BUDGET_BYTES and os.environ.get("MSS_KEEP_DEC_XT", "1") != "0"
        kx0 = {} if (keep_dec and self.final[0].weight.requires_grad) else None
        kx3 = {} if (keep_dec and self.final[3].weight.requires_grad) else None
        if f0 is None:
            f0 = K.conv3x3(dec0, self.final[0].weight, want_stats=train, keep_xt=kx0)
        st_f0 = K.bn_fold(self.final[1], f0, train)
        f1 = K.conv3x3(f0, self.final[3].weight, in_affine=(st_f0.scale, st_f0.shift), in_relu=True, want_stats=train, keep_xt=kx3)
        st_f1 = K.bn_fold(self.final[4], f1, train)
        final_xt = {0: kx0.get("xt") if kx0 else None, 3: kx3.get("xt") if kx3 else None}
        wh, _ = self._heads_weight()
        dec12 = K.conv2d(f1, wh, in_affine=(st_f1.scale, st_f1.shift), in_relu=True)
        C = self.num_classes
        q, _ = heads_layout(C)
        score, logit, label = K.ood_score(dec12.slice(q, C), dec12.slice(0, C) if (want_logit or want_label) else None, size[0], size[1],
                                          want_logit=want_logit, want_label=want_label)
        if want_label:                 # evaluate(): the uint8 argmax of the logits, whether or not they are written
            return score, logit, label
        saved = None
        if keep:
            saved = dict(plan=plan, aspp_xt=aspp_xt, x=x, fx=fx, comp=comp, drop=drop, m2=m2, raw=raw, scale=scale, shift=shift, states=states, pooled_act=pooled_act,
                         u0_rows=u0_rows, dec0=dec0, f0=f0, st_f0=st_f0, f1=f1, st_f1=st_f1, dec12=dec12, size=size, final_xt=final_xt)
        return score, logit, saved

    def _head_backward(self, s, dscore, dlogit, needs):
        names, params = self._head_params()
        need = {n: bool(f) for n, f in zip(names, needs)}
        sink = self.grad_sink

        class _Grads(dict):
            def __setitem__(self, k, v):
                if sink is not None and v is not None and need.get(k):
                    r = sink(k, v)             # a sink may hand back the tensor autograd should get (ddp: its flat-buffer slice)
                    if r is not None:
                        v = r
                dict.__setitem__(self, k, v)
        grads = _Grads()
        try:
            out = self._head_backward_impl(s, dscore, dlogit, names, need, grads)
        except BaseException:
            if sink is not None and hasattr(sink, "abort"):
                sink.abort()       # no collective is started while an exception unwinds (ranks would deadlock)
            raise
        if sink is not None and hasattr(sink, "backward_done"):
            sink.backward_done()
        return out

    def _head_backward_impl(self, s, dscore, dlogit, names, need, grads):
        x, m2, raw, dec0, f0, f1, dec12 = s["x"], s["m2"], s["raw"], s["dec0"], s["f0"], s["f1"], s["dec12"]
        N, h8, w8, h2, w2 = x.N, x.H, x.W, m2.H, m2.W
        OH, OW = s["size"]
        dev = x.buf.device
        dscore = dscore.contiguous() if dscore is not None else None
        dlogit = dlogit.contiguous() if dlogit is not None else None
        C = self.num_classes
        q, Kh = heads_layout(C)
        ddec12 = Act.zeros(N, h2, w2, Kh, dev)
        # both slices always: the tiled kernel writes the whole Kh-channel row (zeros where a gradient is absent)
        K.ood_score_bwd(dec12.slice(q, C), dscore, dlogit, ddec12.slice(q, C), ddec12.slice(0, C), OH, OW)
        aff_f1 = (s["st_f1"].scale, s["st_f1"].shift)
        if need["ood_head.weight"]:
            grads["ood_head.weight"] = K.conv2d_wgrad(f1, ddec12.slice(q, C), C, 256, 1, 1, in_affine=aff_f1,
                                                      in_relu=True)
        if need["final.6.weight"]:
            grads["final.6.weight"] = K.conv2d_wgrad(f1, ddec12.slice(0, C), C, 256, 1, 1, in_affine=aff_f1,
                                                     in_relu=True)
        upstream = [n for n in names if need[n] and not n.startswith(("ood_head", "final.6"))]
        if not upstream:
            return [grads.get(n) for n in names]
        _, wh_flip = self._heads_weight()
        d_act1 = K.conv2d(ddec12, wh_flip)
        # Neither stage of exps/DeepLab.yaml trains `final`: the gradient w.r.t. a BatchNorm's input then has ONE consumer, the data
        # gradient of the 3x3 layer in front of it, and the BatchNorm backward's apply pass rides in that convolution's Winograd
        # input transform (kernels.conv3x3_dgrad_after_bn: df1 / df0 are never written). With `final` trainable: the separate steps.
        aff_f0 = (s["st_f0"].scale, s["st_f0"].shift)
        if need["final.4.weight"] or need["final.4.bias"] or need["final.3.weight"]:
            df1, dg, db = K.bn_relu_backward(d_act1, f1, s["st_f1"], want_param_grads=need["final.4.weight"] or need["final.4.bias"])
            grads["final.4.weight"], grads["final.4.bias"] = dg, db
            if need["final.3.weight"]:
                grads["final.3.weight"] = K.conv3x3_wgrad(f0, df1, 256, 256, in_affine=aff_f0, in_relu=True, xt=s["final_xt"].pop(3, None))
            d_act0 = K.conv3x3(df1, self.final[3].weight, flip=True)
            del df1
        else:
            d_act0 = K.conv3x3_dgrad_after_bn(d_act1, f1, s["st_f1"], self.final[3].weight)
        del d_act1
        upstream = any(need[n] for n in names if n.startswith(("aspp", "bot_")))
        if need["final.1.weight"] or need["final.1.bias"] or need["final.0.weight"]:
            df0, dg, db = K.bn_relu_backward(d_act0, f0, s["st_f0"], want_param_grads=need["final.1.weight"] or need["final.1.bias"])
            grads["final.1.weight"], grads["final.1.bias"] = dg, db
            if need["final.0.weight"]:
                grads["final.0.weight"] = K.conv3x3_wgrad(dec0, df0, 256, 304, xt=s["final_xt"].pop(0, None))
            if not upstream:
                return [grads.get(n) if need[n] else None for n in names]
            ddec0 = K.conv3x3(df0, self.final[0].weight, flip=True)
            del df0
        else:
            if not upstream:
                return [grads.get(n) if need[n] else None for n in names]
            ddec0 = K.conv3x3_dgrad_after_bn(d_act0, f0, s["st_f0"], self.final[0].weight)
        if need["bot_fine.weight"]:
            grads["bot_fine.weight"] = K.conv2d_wgrad(m2, ddec0.slice(0, 48), 48, 128, 1, 1)
        if any(need[n] for n in names if n.startswith(("aspp", "bot_aspp"))):
            d_up = K.upsample_ac_bwd(ddec0.slice(48, 256), h8, w8)
            aff = (s["scale"], s["shift"])
            if need["bot_aspp.weight"]:
                grads["bot_aspp.weight"] = K.conv2d_wgrad(raw, d_up, 256, 1280, 1, 1, in_affine=aff, in_relu=True)
            if any(need[n] for n in names if n.startswith("aspp")):
                d_act = K.conv2d(d_up, K.packed(self.bot_aspp.weight, flip=True))
                states = s["states"]
                plan, comp, fx, drop = s["plan"], s["comp"], s["fx"], s["drop"]
                held = {}          # composed route: this loop's gradients, handed on in its own order once the four are projected
                out = grads if comp is None else held
                # the three dilated branches first (37.7 MB of gradient each), the two 4 MB branches last: under data parallelism the
                # all-reduce of each large gradient runs beside the next branch's weight-gradient GEMMs and only a small bucket
                # is left after the last kernel of the backward (trainer.BACKWARD_ORDER lists the gradients in this order)
                for i in (3, 2, 1, 0):
                    p = f"aspp.features.{i}"
                    sl = raw.slice(256 * (i + 1), 256)
                    want = need[p + ".1.weight"] or need[p + ".1.bias"]
                    draw, dg, db = K.bn_relu_backward(d_act.slice(256 * (i + 1), 256), sl, states[i + 1], want_param_grads=want)
                    out[p + ".1.weight"], out[p + ".1.bias"] = dg, db
                    if need[p + ".0.weight"]:
                        if i == 0 and comp is not None:
                            # the weight gradient of the two K-halves, each with its factor's prologue
                            out[p + ".0.weight"] = torch.cat(
                                [K.conv2d_wgrad(fx.a0, draw, 256, fx.a0.C, 1, 1, in_affine=fx.aff0, in_relu=True),
                                 K.conv2d_wgrad(fx.a1, draw, 256, fx.a1.C, 1, 1, in_affine=fx.aff1, in_relu=True)], dim=1)
                        elif i == 0:
                            out[p + ".0.weight"] = K.conv2d_wgrad(x, draw, 256, 4096, 1, 1)
                        elif plan.dropped:
                            # (its X' is always kept: a step over the X' budget does not take the dropped route)
                            out[p + ".0.weight"] = K.conv3x3_wgrad_dropped(x, draw, 256, 4096, _ASPP_RATES[i - 1], s["aspp_xt"].pop(i), drop)
                        else:
                            out[p + ".0.weight"] = K.conv3x3_wgrad(x, draw, 256, 4096, dil=_ASPP_RATES[i - 1],
                                                                   xt=s["aspp_xt"].pop(i, None))
                if comp is not None:
                    # gradients w.r.t. the composed weights -> gradients w.r.t. the ASPP weights: dW = dWc . M^T, the four of them
                    # (tap-major rows, spatial domain) in ONE product
                    keys = [f"aspp.features.{i}.0.weight" for i in range(4) if f"aspp.features.{i}.0.weight" in held]
                    if keys:
                        flops = 2.0 * sum(held[k].numel() // (held[k].shape[0] if held[k].dim() == 5 else 1) for k in keys) * comp["M"].K
                        with K._Timed("aspp_compose", flops, ("project", len(keys))):
                            for k, g in zip(keys, self._aspp_rows([held[k] for k in keys], comp["M"], dropped=drop)):
                                held[k] = g.dense()
                    for k, g in held.items():
                        grads[k] = g
                # image-pooling branch: the broadcast's transpose is a column sum
                dv = K.colsum(d_act.slice(0, 256))
                want = need["aspp.img_conv.1.weight"] or need["aspp.img_conv.1.bias"]
                du0, dg, db = K.bn_relu_backward(None, None, states[0], want_param_grads=want, x_rows=s["u0_rows"], dy_rows=dv)
                grads["aspp.img_conv.1.weight"], grads["aspp.img_conv.1.bias"] = dg, db
                if need["aspp.img_conv.0.weight"]:
                    grads["aspp.img_conv.0.weight"] = K.conv2d_wgrad(s["pooled_act"], Act(du0.view(N, 1, 1, 256)), 256,
                                                                     4096, 1, 1)
        return [grads.get(n) if need[n] else None for n in names]

    # ---- forward -------------------------------------------------------------------------------------
    def forward(self, inp):
        if not inp.is_cuda:
            raise RuntimeError("DeepWV3Plus (multishiftseg_amd) runs on an MI355X only; there is no CPU path")
        inp = inp.float()
        size = (inp.shape[2], inp.shape[3])
        names, params = self._head_params()
        want_grad = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        if torch.is_grad_enabled():
            self._check_trunk_frozen()
        with K.batched_counters():
            with torch.no_grad():
                x, m2 = self._run_trunk(inp)
            if want_grad:
                score, logit = _HeadFn.apply(self, x, m2, size, *params)
            else:
                with torch.no_grad():
                    score, logit, _ = self._head_forward(x, m2, size, want_logit=self.training or not self.score_only)
        return score, logit

    def evaluate(self, batches, meter=None, seg_meter=None, group=None):
        """The validation / test sweep (train_deeplab.py:223-241, test_deeplab.py:84-102) with no copy to the host: `batches` yields
        (images, target); every anomaly-score map goes to OODMeter.update on the device. Returns meter.compute().
        seg_meter (a metric.SegMeter): the closed-set half as well, from the SAME forward: the score tail also writes the uint8 argmax
        of the logits it interpolates (1 byte per pixel instead of the 76 of the logits, which are not written: score_only or not,
        the sweep never needs them), and that map goes to SegMeter.update. Returns (meter.compute(), seg_meter.compute()).
        Evaluation mode, no gradients; the mode the module was in is restored.
        group (a process group, or True for the default one): the sweep is split over the ranks. Each rank consumes the `batches` it
        is given -- the caller shards them, e.g. ddp.shard_batches(loader) -- and after the loop every rank, one with an empty shard
        too, gathers the OOD keys and sums the confusion matrix (ddp.gather_meters), so every rank returns what one process
        returns over all batches, bit for bit. A rank that raises inside its sweep raises before the collective: its
        peers wait there until the process group's timeout. None: no collective, the sweep of one process."""
        from .metric import OODMeter
        meter = OODMeter() if meter is None else meter
        if seg_meter is not None and seg_meter.n_cl != self.num_classes:
            raise ValueError(f"seg_meter counts {seg_meter.n_cl} classes, the model predicts {self.num_classes}")
        was = self.training
        self.eval()
        try:
            for images, target in batches:
                if not images.is_cuda:
                    raise RuntimeError("DeepWV3Plus (multishiftseg_amd) runs on an MI355X only; there is no CPU path")
                images = images.float()
                size = (images.shape[2], images.shape[3])
                with K.batched_counters(), torch.no_grad():
                    x, m2 = self._run_trunk(images)
                    score, _, label = self._head_forward(x, m2, size, want_logit=False, want_label=seg_meter is not None)
                meter.update(score, target)
                if seg_meter is not None:
                    seg_meter.update(label, target)
        finally:
            self.train(was)
        if group is not None:
            from . import ddp
            ddp.gather_meters(group, meter, seg_meter)
        if seg_meter is None:
            return meter.compute()
        return meter.compute(), seg_meter.compute()
