"""Mask2Former's GMA transformer decoder: forward only by default, trainable on request.

Host-side mirror of ``MultiScaleMaskedTransformerDecoder_GMA``
(lib/network/mask2former/modeling/transformer_decoder/mask2former_transformer_decoder.py:280-573): same constructor
keywords, same parameter names and shapes (a reference ``state_dict`` of the sub-module loads with ``strict=True``, the unused
``fusion_layer`` included), same ``forward(x, mask_features, mask=None)`` returning ``pred_logits``, ``pred_masks``,
``pred_logits_ood``, ``pred_masks_ood`` and ``aux_outputs``. The ``nn.MultiheadAttention`` / ``nn.Linear`` / ``nn.LayerNorm``
children are parameter containers only; their ``forward`` is never called.

What runs (all in libmss_hip.so; tokens are batch-major [B, rows, 256] inside, the reference's [rows, B, 256] never exists):
  * per level, once: input_proj (1x1 conv, level embedding folded into its bias) -> src; src + pos;
  * per layer: the key projections of the foreground and the background attention as ONE product over the stacked weights from
    src + pos, the value projections likewise from src, the two query projections likewise from tgt + query_pos;
    csrc/m2f_attn.hip: mask bits + rescue flags from the previous step's pixel-major mask logits, then both masked attentions in
    one launch; the two out_proj as one K = 512 product with the summed bias; residual + LayerNorm (add_layernorm);
    self-attention among the queries on the same attention kernel without a mask; the FFN with the ReLU in the GEMM epilogue;
  * per prediction step (10): decoder_norm, class_embed + class_embed2 as one (zero-padded) product, the mask_embed MLP, and
    the mask logits as one batched GEMM written pixel-major (kernels.m2f_mask_logits_act). forward_prediction_heads and
    forward_ood_heads share decoder_norm and mask_embed, so pred_masks_ood IS pred_masks (the same tensor object).

Supported: pre_norm=False, hidden_dim=256, nheads=8, mask_dim a multiple of 16, <= 128 queries, float32 CUDA inputs. Eval and
"stage 1" training, where only class_embed2 receives a gradient (train_m2f.py, M2F.yaml:9); every other trainable parameter
under an enabled grad mode raises, as does anything else outside this list. set_trainable() opts in to the differentiable path
of stage 2 (_forward_train: the same arithmetic on autograd nodes, the attention's backward in csrc/m2f_attn.hip). forward(...,
semantic=(Hp, Wp, H, W)) adds what stage 1 trains on: "sem_seg" and a differentiable "ood_score" (kernels.m2f_semantic_inference).
There is no CPU path and no torch fallback.
"""
import torch
from torch import nn

from . import kernels as K
from .linear import _rows, ffn_relu, linear
from .msdeformattn_encoder import PositionEmbeddingSine


class _MLP(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, num_layers):
        super().__init__()
        self.num_layers = num_layers
        h = [hidden_dim] * (num_layers - 1)
        self.layers = nn.ModuleList(nn.Linear(n, k) for n, k in zip([input_dim] + h, h + [output_dim]))


class _SelfAttentionLayer(nn.Module):
    def __init__(self, d_model, nhead):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d_model, nhead, dropout=0.0)
        self.norm = nn.LayerNorm(d_model)
        _xavier(self)


class _GlobalCrossAttentionLayer(nn.Module):
    def __init__(self, d_model, nhead):
        super().__init__()
        self.multihead_attn_foreground = nn.MultiheadAttention(d_model, nhead, dropout=0.0)
        self.multihead_attn_background = nn.MultiheadAttention(d_model, nhead, dropout=0.0)
        self.norm = nn.LayerNorm(d_model)
        self.fusion_layer = nn.Conv2d(200, 100, kernel_size=1)     # present in the reference's state_dict, used by nothing
        _xavier(self)


class _FFNLayer(nn.Module):
    def __init__(self, d_model, dim_feedforward):
        super().__init__()
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm = nn.LayerNorm(d_model)
        _xavier(self)


def _xavier(module):
    for p in module.parameters():
        if p.dim() > 1:
            nn.init.xavier_uniform_(p)


def _sig(params):
    return tuple((p._version, p.data_ptr()) for p in params)


class MultiScaleMaskedTransformerDecoder_GMA(nn.Module):
    _version = 2

    def __init__(self, in_channels, mask_classification=True, *, num_classes, hidden_dim, num_queries, nheads, dim_feedforward,
                 dec_layers, pre_norm, mask_dim, enforce_input_project):
        super().__init__()
        if not mask_classification:
            raise NotImplementedError("Only support mask classification model")
        if pre_norm:
            raise NotImplementedError("transformer_decoder (multishiftseg_amd): pre_norm=True is not implemented")
        if hidden_dim != 256 or nheads != 8:
            raise NotImplementedError("transformer_decoder (multishiftseg_amd): the attention kernel is built for hidden_dim=256, "
                                      f"nheads=8 (head dimension 32), got {hidden_dim} / {nheads}")
        if not 1 <= num_queries <= 128:
            raise NotImplementedError(f"transformer_decoder (multishiftseg_amd): 1 .. 128 queries, got {num_queries}")
        if mask_dim % 16 or mask_dim <= 64 or dim_feedforward % 16 or dim_feedforward <= 64 or in_channels < 1 or 2 * (num_classes + 1) > 128:
            raise NotImplementedError("transformer_decoder (multishiftseg_amd): mask_dim and dim_feedforward must be multiples of 16 "
                                      "above 64, and at most 63 classes")
        self.mask_classification = mask_classification
        self.pe_layer = PositionEmbeddingSine(hidden_dim // 2, normalize=True)
        self.num_heads = nheads
        self.num_layers = dec_layers
        self.transformer_self_attention_layers = nn.ModuleList(_SelfAttentionLayer(hidden_dim, nheads) for _ in range(dec_layers))
        self.transformer_cross_attention_layers = nn.ModuleList(_GlobalCrossAttentionLayer(hidden_dim, nheads) for _ in range(dec_layers))
        self.transformer_ffn_layers = nn.ModuleList(_FFNLayer(hidden_dim, dim_feedforward) for _ in range(dec_layers))
        self.decoder_norm = nn.LayerNorm(hidden_dim)
        self.num_queries = num_queries
        self.query_feat = nn.Embedding(num_queries, hidden_dim)
        self.query_embed = nn.Embedding(num_queries, hidden_dim)
        self.num_feature_levels = 3
        self.level_embed = nn.Embedding(self.num_feature_levels, hidden_dim)
        self.input_proj = nn.ModuleList()
        for _ in range(self.num_feature_levels):
            if in_channels != hidden_dim or enforce_input_project:
                conv = nn.Conv2d(in_channels, hidden_dim, kernel_size=1)
                nn.init.kaiming_uniform_(conv.weight, a=1)             # fvcore c2_xavier_fill
                nn.init.constant_(conv.bias, 0)
                self.input_proj.append(conv)
            else:
                self.input_proj.append(nn.Sequential())
        self.class_embed = nn.Linear(hidden_dim, num_classes + 1)
        self.mask_embed = _MLP(hidden_dim, hidden_dim, mask_dim, 3)
        self.class_embed2 = nn.Linear(hidden_dim, num_classes + 1)
        self._stacks = {}
        self._pos_cache = {}
        self._trainable = False

    def set_trainable(self, flag=True):
        """Opt in to (or out of) the differentiable path: with the switch on and grad mode enabled, forward() runs on autograd
        nodes over the same kernels and every parameter the reference's autograd reaches (all but the unused fusion_layer), x[i]
        and mask_features receive gradients. Off (the default) the module is forward-only apart from class_embed2, as before;
        under torch.no_grad() the switch makes no difference."""
        self._trainable = bool(flag)
        return self

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        version = local_metadata.get("version", None)
        if version is None or version < 2:                              # the reference's rename of version-1 checkpoints
            for k in list(state_dict.keys()):
                if k.startswith(prefix) and "static_query" in k:
                    state_dict[k.replace("static_query", "query_feat")] = state_dict.pop(k)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    # ---- GEMMs ------------------------------------------------------------------------------------------------------------
    def _stack(self, name, params, make):
        """(packed weight, bias) of a product over several parameters' weights side by side, cached until one of them changes."""
        key = _sig(params)
        ent = self._stacks.get(name)
        if ent is None or ent[0] != key:
            with torch.no_grad():
                w, b = make()
                w = w.contiguous().float()
                ent = self._stacks[name] = (key, K.pack_weight(w.view(w.shape[0], w.shape[1], 1, 1)), b.contiguous().float())
        return ent[1], ent[2]

    @staticmethod
    def _gemm(x, pw, bias, relu=False):
        """x [..., c] -> [..., k] on the fp32 MFMA GEMM (bias and ReLU in its epilogue)."""
        k = pw.K + (pw.tail.K if pw.tail is not None else 0)
        out = torch.empty(x.shape[:-1] + (k,), device=x.device, dtype=torch.float32)
        K.conv2d(_rows(x, x.shape[-1]), pw, out_affine=(K.ones(k, x.device), bias), out_relu=relu, out=_rows(out, k))
        return out

    def _lin(self, name, x, lin, relu=False):
        pw, b = self._stack(name, (lin.weight, lin.bias), lambda: (lin.weight, lin.bias))
        return self._gemm(x, pw, b, relu)

    # ---- pieces -----------------------------------------------------------------------------------------------------------
    def _cross_stacks(self, i):
        """Layer i's cross-attention products: (q, k, v, out) over [foreground; background]."""
        ca = self.transformer_cross_attention_layers[i]
        fg, bg = ca.multihead_attn_foreground, ca.multihead_attn_background
        C = fg.embed_dim
        ins = (fg.in_proj_weight, fg.in_proj_bias, bg.in_proj_weight, bg.in_proj_bias)
        outs = (fg.out_proj.weight, fg.out_proj.bias, bg.out_proj.weight, bg.out_proj.bias)

        def part(j):
            return lambda: (torch.cat((fg.in_proj_weight[j * C:(j + 1) * C], bg.in_proj_weight[j * C:(j + 1) * C]), 0),
                            torch.cat((fg.in_proj_bias[j * C:(j + 1) * C], bg.in_proj_bias[j * C:(j + 1) * C]), 0))
        return (self._stack(f"ca{i}.q", ins, part(0)), self._stack(f"ca{i}.k", ins, part(1)), self._stack(f"ca{i}.v", ins, part(2)),
                self._stack(f"ca{i}.o", outs, lambda: (torch.cat((fg.out_proj.weight, bg.out_proj.weight), 1),
                                                       fg.out_proj.bias + bg.out_proj.bias)))

    def _self_stacks(self, i):
        sa = self.transformer_self_attention_layers[i].self_attn
        C = sa.embed_dim
        ins = (sa.in_proj_weight, sa.in_proj_bias)
        return (self._stack(f"sa{i}.qk", ins, lambda: (sa.in_proj_weight[:2 * C], sa.in_proj_bias[:2 * C])),
                self._stack(f"sa{i}.v", ins, lambda: (sa.in_proj_weight[2 * C:], sa.in_proj_bias[2 * C:])),
                self._stack(f"sa{i}.o", (sa.out_proj.weight, sa.out_proj.bias), lambda: (sa.out_proj.weight, sa.out_proj.bias)))

    def _class_logits(self, dn):
        """class_embed and class_embed2 as one product, zero-padded to 128 outputs (the MFMA GEMM takes more than 64 outputs
        in multiples of 16); the only place a gradient may enter (stage 1: class_embed2)."""
        c1, c2 = self.class_embed, self.class_embed2
        n = c1.out_features
        if torch.is_grad_enabled() and (c2.weight.requires_grad or c2.bias.requires_grad):
            pad_w = c2.weight.new_zeros((128 - 2 * n, c2.in_features))
            w = torch.cat((c1.weight.detach(), c2.weight, pad_w), 0)
            b = torch.cat((c1.bias.detach(), c2.bias, pad_w[:, 0]), 0)
            y = linear(dn, w, b)
            return y[..., :n].detach().contiguous(), y[..., n:2 * n].contiguous()
        else:
            pw, b = self._stack("class", (c1.weight, c1.bias, c2.weight, c2.bias), lambda: (
                torch.cat((c1.weight, c2.weight, c1.weight.new_zeros((128 - 2 * n, c1.in_features))), 0),
                torch.cat((c1.bias, c2.bias, c1.bias.new_zeros(128 - 2 * n)), 0)))
            y = self._gemm(dn, pw, b)
        return y[..., :n].contiguous(), y[..., n:2 * n].contiguous()

    def _mask_step(self, tgt, feat, ldq):
        """The frozen part of forward_prediction_heads / forward_ood_heads (:524-560), which share decoder_norm and mask_embed:
        -> decoder_norm(tgt), pixel-major mask logits [B, h4, w4, ldq]."""
        dn = K.add_layernorm(tgt, None, self.decoder_norm)
        me = dn
        for j, lin in enumerate(self.mask_embed.layers):
            me = self._lin(f"mlp{j}", me, lin, relu=j < self.mask_embed.num_layers - 1)
        return dn, K.m2f_mask_logits_act(me, feat, ldq)

    def _check_grad_mode(self):
        if not torch.is_grad_enabled():
            return
        allowed = {id(self.class_embed2.weight), id(self.class_embed2.bias)}
        bad = [n for n, p in self.named_parameters() if p.requires_grad and id(p) not in allowed]
        if bad:
            raise NotImplementedError("transformer_decoder (multishiftseg_amd) is forward-only apart from class_embed2 (stage 1): freeze "
                                      f"the other parameters or call under torch.no_grad(); trainable: {bad[:4]} ... ({len(bad)})")

    # ---- reference API ----------------------------------------------------------------------------------------------------
    def forward(self, x, mask_features, mask=None, *, fuse_score=None, return_attn_bits=False, semantic=None, sem_seg=False):
        """As the reference's forward. fuse_score=(H, W): the last step's pixel-major mask logits go straight to
        kernels.m2f_score_fused with pred_logits_ood; the anomaly score [B, H, W] is returned as "ood_score" and the last step's
        NCHW "pred_masks" / "pred_masks_ood" are not materialised (None). fuse_score=(Hp, Wp, H, W): upsample to the padded image
        size (Hp, Wp) and keep the top-left (H, W) of it (maskformer_model.py:264-277 + sem_seg_postprocess). return_attn_bits: "attn_bits" = per layer the packed
        mask words [B, 2, HW, ceil(Q/32)] (int32; bit q of [b, 0 | 1, key] set = query q does not attend to that key in the
        foreground | background attention) as the attention kernel applied them, i.e. after the rescue rule.
        semantic=(Hp, Wp, H, W): the dict gains "sem_seg" [B, min(C,19), H, W] (MaskFormer.semantic_inference of pred_logits on the
        last step's masks upsampled to (Hp, Wp), cropped to (H, W)) and "ood_score" [B, H, W] (train_m2f.py:387-407 of
        pred_logits_ood on the same upsampled masks), both from the last step's pixel-major logits through
        kernels.m2f_semantic_inference. "ood_score" is attached to pred_logits_ood where class_embed2 requires grad (stage 1);
        "sem_seg" never requires grad. Not together with fuse_score, which names the same key.
        sem_seg=True with fuse_score=(Hp, Wp, H, W), evaluation only: the dict also gains "sem_seg" as above, from the same last-step
        logits the fused score read -- the evaluation sweep's closed-set prediction beside the UNCHANGED fused "ood_score" (the score of
        `semantic` is the stage-1 form of the same quantity and differs from the fused one in the last bits)."""
        del mask                                                     # "disable mask, it does not affect performance" (:445)
        if semantic is not None and (fuse_score is not None or len(tuple(semantic)) != 4):
            raise ValueError("semantic=(Hp, Wp, H, W), and not together with fuse_score: both name \"ood_score\"")
        if sem_seg and (fuse_score is None or len(tuple(fuse_score)) != 4 or (self._trainable and torch.is_grad_enabled())):
            raise ValueError("sem_seg=True goes with fuse_score=(Hp, Wp, H, W) on the evaluation path")
        if len(x) != self.num_feature_levels:
            raise ValueError(f"expected {self.num_feature_levels} feature levels, got {len(x)}")
        if not mask_features.is_cuda or not all(t.is_cuda for t in x):
            raise RuntimeError("MultiScaleMaskedTransformerDecoder_GMA (multishiftseg_amd) runs on an MI355X only; there is no CPU path")
        if self._trainable and torch.is_grad_enabled():
            return self._forward_train(x, mask_features, fuse_score, return_attn_bits, semantic)
        if mask_features.requires_grad or any(t.requires_grad for t in x):
            if torch.is_grad_enabled():
                raise NotImplementedError("transformer_decoder (multishiftseg_amd): no backward to the inputs (forward only)")
        self._check_grad_mode()
        with torch.no_grad():
            state = self._forward_frozen(x, mask_features, fuse_score is not None)
        out = self._finish(state, fuse_score, return_attn_bits, semantic)
        if sem_seg:
            Hp, Wp, H, W = (int(v) for v in fuse_score)
            with torch.no_grad():
                out["sem_seg"] = K.m2f_semantic_inference(out["pred_logits"], state[2], (Hp, Wp), (H, W), Q=out["pred_logits"].shape[1])
        return out

    def _position(self, x):
        """[1, hw, C] position code of a level, kept per (size, device): it depends on nothing else."""
        key = (x.shape[-2], x.shape[-1], str(x.device))
        pos = self._pos_cache.get(key)
        if pos is None:
            pos = self._pos_cache[key] = self.pe_layer(x[:1]).flatten(2).transpose(1, 2).contiguous()
        return pos

    def _forward_frozen(self, x, mask_features, skip_last_nchw):
        """Everything but the class heads (nothing here depends on class_embed2) -> per prediction step decoder_norm(tgt) and
        the NCHW masks, the last step's pixel-major mask logits, the mask words of every layer."""
        B = x[0].shape[0]
        Q, L = self.num_queries, self.num_feature_levels
        C = self.decoder_norm.normalized_shape[0]
        dev = x[0].device
        ldq = (Q + 3) // 4 * 4
        sizes, src, kin = [], [], []
        for i in range(L):
            h, w = x[i].shape[-2:]
            sizes.append((h, w))
            xa = K.nchw_to_act(x[i])
            lvl = self.level_embed.weight[i]
            proj = self.input_proj[i]
            if isinstance(proj, nn.Conv2d):
                pw, b = self._stack(f"in{i}", (proj.weight, proj.bias, self.level_embed.weight),
                                    lambda proj=proj, lvl=lvl: (proj.weight.view(proj.out_channels, -1), proj.bias + lvl))
                s = K.conv2d(xa, pw, out_affine=(K.ones(C, dev), b)).buf.view(B, h * w, C)
            else:
                if xa.ld != C:
                    raise ValueError(f"level {i}: {x[i].shape[1]} channels without an input projection, expected {C}")
                s = xa.buf.view(B, h * w, C) + lvl
            src.append(s)
            kin.append(s + self._position(x[i]))
        feat = K.nchw_to_act(mask_features)
        if feat.C != self.mask_embed.layers[-1].out_features:
            raise ValueError(f"mask_features has {mask_features.shape[1]} channels, mask_embed produces {self.mask_embed.layers[-1].out_features}")
        qpos = self.query_embed.weight.float().unsqueeze(0)                    # [1, Q, C]
        tgt = self.query_feat.weight.float().unsqueeze(0).repeat(B, 1, 1).contiguous()
        dn, logits = self._mask_step(tgt, feat, ldq)
        norms, masks, bits_used = [dn], [K.nhwc_to_nchw(K.Act(logits, C=Q))], []
        for i in range(self.num_layers):
            lv = i % L
            h, w = sizes[lv]
            bits, allowed = K.m2f_attn_mask_bits(logits, Q, (h, w))
            bits_used.append((bits, allowed))
            (qw, qb), (kw, kb), (vw, vb), (ow, ob) = self._cross_stacks(i)
            ca = self.transformer_cross_attention_layers[i]
            qp = self._gemm(tgt + qpos, qw, qb)
            kp = self._gemm(kin[lv], kw, kb)
            vp = self._gemm(src[lv], vw, vb)
            att = K.m2f_masked_attention(qp.view(B * Q, 2 * C), kp.view(B * h * w, 2 * C), vp.view(B * h * w, 2 * C), B, Q, h * w, A=2,
                                         bits=bits, allowed=allowed)
            tgt = K.add_layernorm(tgt, self._gemm(att.view(B, Q, 2 * C), ow, ob), ca.norm)
            sl = self.transformer_self_attention_layers[i]
            (qkw, qkb), (svw, svb), (sow, sob) = self._self_stacks(i)
            qk = self._gemm(tgt + qpos, qkw, qkb).view(B * Q, 2 * C)
            sv = self._gemm(tgt, svw, svb).view(B * Q, C)
            att = K.m2f_masked_attention(qk[:, :C], qk[:, C:], sv, B, Q, Q, A=1, chunks=1)
            tgt = K.add_layernorm(tgt, self._gemm(att.view(B, Q, C), sow, sob), sl.norm)
            ffn = self.transformer_ffn_layers[i]
            hid = self._lin(f"ffn{i}.1", tgt, ffn.linear1, relu=True)
            tgt = K.add_layernorm(tgt, self._lin(f"ffn{i}.2", hid, ffn.linear2), ffn.norm)
            dn, logits = self._mask_step(tgt, feat, ldq)
            norms.append(dn)
            last = i + 1 == self.num_layers
            masks.append(None if last and skip_last_nchw else K.nhwc_to_nchw(K.Act(logits, C=Q)))
        return norms, masks, logits, bits_used

    def _forward_train(self, x, mask_features, fuse_score, return_attn_bits, semantic=None):
        """The differentiable path (set_trainable): _forward_frozen's arithmetic on autograd nodes -- linear / ffn_relu /
        add_layernorm, kernels.masked_attention, kernels.mask_logits; the stacked projections are torch.cat of the live parameters,
        so autograd splits their gradients; the mask bits come from the detached logits. fuse_score stays inference-only here: the
        anomaly score is computed from detached tensors and the last step's NCHW masks are still materialised."""
        B = x[0].shape[0]
        Q, L = self.num_queries, self.num_feature_levels
        C = self.decoder_norm.normalized_shape[0]
        ldq = (Q + 3) // 4 * 4
        sizes, src, kin = [], [], []
        for i in range(L):
            h, w = x[i].shape[-2:]
            sizes.append((h, w))
            xa = K._NchwToRowsFn.apply(x[i])                                     # [B, h, w, Cp]
            lvl = self.level_embed.weight[i]
            proj = self.input_proj[i]
            if isinstance(proj, nn.Conv2d):
                wgt = proj.weight.view(proj.out_channels, -1)
                if xa.shape[-1] != wgt.shape[1]:
                    wgt = nn.functional.pad(wgt, (0, xa.shape[-1] - wgt.shape[1]))
                s = linear(xa.view(B, h * w, -1), wgt, proj.bias + lvl)
            else:
                if xa.shape[-1] != C:
                    raise ValueError(f"level {i}: {x[i].shape[1]} channels without an input projection, expected {C}")
                s = xa.view(B, h * w, C) + lvl
            src.append(s)
            kin.append(s + self._position(x[i]))
        if mask_features.shape[1] != self.mask_embed.layers[-1].out_features:
            raise ValueError(f"mask_features has {mask_features.shape[1]} channels, mask_embed produces {self.mask_embed.layers[-1].out_features}")
        feat = K.Act(K._NchwToRowsFn.apply(mask_features), C=mask_features.shape[1])
        c1, c2 = self.class_embed, self.class_embed2
        n = c1.out_features
        pad_w = c1.weight.new_zeros((128 - 2 * n, c1.in_features))
        cls_w, cls_b = torch.cat((c1.weight, c2.weight, pad_w), 0), torch.cat((c1.bias, c2.bias, pad_w[:, 0]), 0)
        cls, cls_ood, masks, bits_used = [], [], [], []

        def heads(tgt):
            dn = K.add_layernorm(tgt, None, self.decoder_norm)
            y = linear(dn, cls_w, cls_b)
            cls.append(y[..., :n].contiguous())
            cls_ood.append(y[..., n:2 * n].contiguous())
            me = dn
            for j, lin in enumerate(self.mask_embed.layers):
                me = linear(me, lin.weight, lin.bias, relu=j < self.mask_embed.num_layers - 1)
            logits = K.mask_logits(me, feat, ldq)
            masks.append(K._RowsToNchwFn.apply(logits, Q))
            return logits

        qpos = self.query_embed.weight.float().unsqueeze(0)
        tgt = self.query_feat.weight.float().unsqueeze(0).repeat(B, 1, 1)
        logits = heads(tgt)
        for i in range(self.num_layers):
            lv = i % L
            h, w = sizes[lv]
            bits, allowed = K.m2f_attn_mask_bits(logits.detach(), Q, (h, w))
            bits_used.append((bits, allowed))
            ca = self.transformer_cross_attention_layers[i]
            fg, bg = ca.multihead_attn_foreground, ca.multihead_attn_background

            def part(j):
                return (torch.cat((fg.in_proj_weight[j * C:(j + 1) * C], bg.in_proj_weight[j * C:(j + 1) * C]), 0),
                        torch.cat((fg.in_proj_bias[j * C:(j + 1) * C], bg.in_proj_bias[j * C:(j + 1) * C]), 0))
            qp = linear(tgt + qpos, *part(0))
            kp = linear(kin[lv], *part(1))
            vp = linear(src[lv], *part(2))
            att = K.masked_attention(qp.view(B * Q, 2 * C), kp.view(B * h * w, 2 * C), vp.view(B * h * w, 2 * C), B, Q, h * w, A=2,
                                     bits=bits, allowed=allowed)
            o = linear(att.view(B, Q, 2 * C), torch.cat((fg.out_proj.weight, bg.out_proj.weight), 1), fg.out_proj.bias + bg.out_proj.bias)
            tgt = K.add_layernorm(tgt, o, ca.norm)
            sl = self.transformer_self_attention_layers[i]
            sa = sl.self_attn
            qk = linear(tgt + qpos, sa.in_proj_weight[:2 * C], sa.in_proj_bias[:2 * C]).view(B * Q, 2 * C)
            sv = linear(tgt, sa.in_proj_weight[2 * C:], sa.in_proj_bias[2 * C:]).view(B * Q, C)
            att = K.masked_attention(qk[:, :C], qk[:, C:], sv, B, Q, Q, A=1, chunks=1)
            tgt = K.add_layernorm(tgt, linear(att.view(B, Q, C), sa.out_proj.weight, sa.out_proj.bias), sl.norm)
            ffn = self.transformer_ffn_layers[i]
            tgt = K.add_layernorm(tgt, ffn_relu(tgt, ffn.linear1, ffn.linear2), ffn.norm)
            logits = heads(tgt)
        return self._assemble(cls, cls_ood, masks, logits.detach(), bits_used, fuse_score, return_attn_bits, semantic)

    def _finish(self, state, fuse_score, return_attn_bits, semantic=None):
        norms, masks, last_logits, bits_used = state
        cls, cls_ood = [], []
        for dn in norms:
            c, co = self._class_logits(dn)
            cls.append(c)
            cls_ood.append(co)
        return self._assemble(cls, cls_ood, masks, last_logits, bits_used, fuse_score, return_attn_bits, semantic)

    @staticmethod
    def _assemble(cls, cls_ood, masks, last_logits, bits_used, fuse_score, return_attn_bits, semantic=None):
        # the reference runs forward_ood_heads after every layer but not on the initial queries: its OOD lists are one short, and
        # _set_aux_loss zips them against the full lists (:502-521, 563-571) -- aux entry j pairs step j with the OOD heads of layer j
        ood_c, ood_m = cls_ood[1:], masks[1:]
        out = {
            "pred_logits": cls[-1], "pred_masks": masks[-1],
            "aux_outputs": [{"pred_logits": a, "pred_masks": b, "pred_logits_ood": c, "pred_masks_ood": d}
                            for a, b, c, d in zip(cls[:-1], masks[:-1], ood_c[:-1], ood_m[:-1])],
            "pred_logits_ood": ood_c[-1], "pred_masks_ood": ood_m[-1],
        }
        if fuse_score is not None:
            fs = tuple(fuse_score)
            out["ood_score"] = K.m2f_score_fused(ood_c[-1].detach(), last_logits, fs[:2], fs[2:] if len(fs) == 4 else None)
        if semantic is not None:
            Hp, Wp, H, W = (int(v) for v in semantic)
            out["sem_seg"], out["ood_score"] = K.m2f_semantic_inference(cls[-1], last_logits, (Hp, Wp), (H, W), class_logits_ood=ood_c[-1],
                                                                        Q=cls[-1].shape[1])
        if return_attn_bits:
            out["attn_bits"] = [bits & allowed.unsqueeze(2) for bits, allowed in bits_used]
        return out
