"""GPU: the Mask2Former GMA transformer decoder on HIP (multishiftseg_amd/transformer_decoder.py, csrc/m2f_attn.hip) -- the two new
kernels alone, then the whole module against the reference fixture and against the stock-torch restatement
(tests/ref_transformer_decoder.py, pinned to the reference by tests/test_transformer_decoder_cpu.py) at real sizes."""
import numpy as np
import pytest
import torch

import poison
import ref_transformer_decoder as R
from conftest import golden

pytestmark = pytest.mark.gpu

GEOM = dict(num_classes=19, hidden_dim=256, num_queries=100, nheads=8, dim_feedforward=2048, dec_layers=9, pre_norm=False,
            mask_dim=256, enforce_input_project=False)


def unpack(bits, Q):
    """int32 words [..., W] -> bool [..., Q]."""
    sh = torch.arange(32, device=bits.device, dtype=torch.int32)
    return ((bits.unsqueeze(-1) >> sh) & 1).flatten(-2)[..., :Q].bool()


def pack(mask):
    """bool [..., Q] -> int32 words [..., ceil(Q/32)]."""
    Q = mask.shape[-1]
    W = (Q + 31) // 32
    m = torch.zeros(mask.shape[:-1] + (W * 32,), dtype=torch.int64, device=mask.device)
    m[..., :Q] = mask
    words = (m.view(mask.shape[:-1] + (W, 32)) << torch.arange(32, device=mask.device)).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).contiguous()


# ---- 3. the mask-bits kernel alone -----------------------------------------------------------------------------------------------
# (source size, level size, B, Q, seed, grid): grid=True draws logits on the 1/8 grid, for which the bilinear blend of a dyadic
# size ratio is exact in fp32 whatever the contraction (zeros of the blend are then exact zeros: masked in neither row);
# grid=False draws plain floats at the small sizes, with seeds checked on the CPU to put no interpolated fp64 value in
# 0 < |x| < 1e-5 max|x| -- asserted below, so the allowance for a differing fp32 contraction is never used.
BITS_CASES = [((24, 40), (3, 5), 2, 100, 1, True), ((24, 40), (3, 5), 2, 37, 2, False), ((176, 176), (22, 22), 2, 100, 3, True),
              ((176, 176), (44, 44), 1, 37, 4, True), ((176, 176), (88, 88), 2, 100, 5, True), ((256, 512), (128, 256), 1, 100, 6, True),
              ((25, 37), (7, 9), 2, 100, 7, False), ((25, 37), (7, 9), 1, 37, 8, False), ((24, 40), (12, 20), 2, 100, 9, False)]


def bits_case_logits(src, B, Q, seed, grid):
    """[B, Q, hm, wm] float32 on the CPU: N(0, 5), a 6 x 6 patch and every 97th value exactly 0, query 3 negative everywhere,
    query 5 positive everywhere (the two rescue flags)."""
    g = torch.Generator().manual_seed(seed)
    x = 5.0 * torch.randn((B, Q, src[0], src[1]), generator=g)
    if grid:
        x = torch.round(x * 8) / 8
    x[:, :, 2:8, 3:9] = 0.0
    x.view(-1)[::97] = 0.0
    x[:, 3] = -x[:, 3].abs() - 0.125
    x[:, 5] = x[:, 5].abs() + 0.125
    return x


@pytest.mark.parametrize("src,dst,B,Q,seed,grid", BITS_CASES)
def test_mask_bits_kernel_is_exact(src, dst, B, Q, seed, grid):
    from multishiftseg_amd import kernels as K
    x = bits_case_logits(src, B, Q, seed, grid).cuda()
    ldq = (Q + 3) // 4 * 4
    nhwc = torch.zeros((B, src[0], src[1], ldq), device="cuda")
    nhwc[..., :Q] = x.permute(0, 2, 3, 1)
    bits, allowed = K.m2f_attn_mask_bits(nhwc, Q, dst)
    torch.cuda.synchronize()
    it32 = R.interp_logits(x, dst).flatten(2)                       # [B, Q, hw]
    it64 = R.interp_logits(x.double(), dst).flatten(2)
    near = (it64.abs() < 1e-5 * it64.abs().max()) & (it64 != 0)
    assert int(near.sum()) == 0, "the committed inputs must hold no value at rounding level"
    assert int((it32 == 0).sum()) >= B * Q // 2                       # exact zeros are exercised
    want = torch.stack((it32 < 0, it32 > 0), 1).transpose(2, 3)     # [B, 2, hw, Q]
    got = unpack(bits, Q)
    diff = got != want
    assert int(diff.sum()) == 0, f"{int(diff.sum())} differing bits, first at {diff.nonzero()[0].tolist()}"
    want_allowed = (~want).any(2)                                   # [B, 2, Q]
    assert torch.equal(unpack(allowed, Q), want_allowed)
    assert not want_allowed[:, 0, 3].any() and not want_allowed[:, 1, 5].any() and want_allowed[:, 0, 5].all()
    if Q % 32:                                                       # padding bits of the last word stay clear in the rows
        assert int(((bits[..., -1].to(torch.int64) & 0xFFFFFFFF) >> (Q % 32)).sum()) == 0


# ---- 4. the attention kernel alone -----------------------------------------------------------------------------------------------
def attention_reference(q, k, v, mask, B, Q, NK, A, dtype):
    """softmax(q k^T / sqrt(32) + mask) v per (image, attention, head) in `dtype`; mask bool [B, A, Q, NK] (True = not allowed)."""
    out = torch.empty((B * Q, A * 256), dtype=dtype, device=q.device)
    for a in range(A):
        sl = slice(a * 256, (a + 1) * 256)
        qq = q[:, sl].to(dtype).view(B, Q, 8, 32).transpose(1, 2)
        kk = k[:, sl].to(dtype).view(B, NK, 8, 32).transpose(1, 2)
        vv = v[:, sl].to(dtype).view(B, NK, 8, 32).transpose(1, 2)
        s = torch.matmul(qq * (32 ** -0.5), kk.transpose(2, 3))
        if mask is not None:
            s = s.masked_fill(mask[:, a].unsqueeze(1), float("-inf"))
        out[:, sl] = torch.matmul(torch.softmax(s, -1), vv).transpose(1, 2).reshape(B * Q, 256)
    return out


ATTN_CASES = [(1, 100, 15, 2, 1), (2, 37, 100, 1, 1), (1, 100, 100, 1, 4), (1, 100, 7744, 2, 1), (1, 100, 7744, 2, None), (1, 37, 1936, 2, 5),
              (16, 100, 7744, 2, None), (16, 37, 484, 2, None), (1, 100, 32768, 2, None), (1, 128, 32768, 1, 200)]


@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("B,Q,NK,A,chunks", ATTN_CASES)
def test_masked_attention_kernel(B, Q, NK, A, chunks, masked):
    """Bound: 4 x the error of the same formula evaluated by torch in fp32 on the same input (measured here), against fp64.
    Mask rows: random at 50 %; query 1 sees only the last 3 keys (fully masked in every chunk but the last); query 2 fully
    masked and rescued through its `allowed` bit. Twice for bit-reproducibility, once more on a NaN-filled workspace."""
    from multishiftseg_amd import _lib, kernels as K
    g = torch.Generator(device="cuda").manual_seed(1000 + NK + Q)
    q = torch.randn((B * Q, A * 256), device="cuda", generator=g)
    k = torch.randn((B * NK, A * 256), device="cuda", generator=g)
    v = torch.randn((B * NK, A * 256), device="cuda", generator=g)
    bits = allowed = mask = None
    if masked:
        mask = torch.rand((B, A, Q, NK), device="cuda", generator=g) < 0.5
        mask[:, :, 1, :] = True
        mask[:, :, 1, max(0, NK - 3):] = False
        mask[:, :, 2, :] = True
        mask[:, :, 0, 0] = False                                     # every other row keeps at least one key
        mask[:, :, 3:, 0] = False
        bits = pack(mask.transpose(2, 3).contiguous())               # [B, A, NK, W]
        ok = torch.ones((B, A, Q), dtype=torch.bool, device="cuda")
        ok[:, :, 2] = False
        allowed = pack(ok)
        mask = mask.clone()
        mask[:, :, 2, :] = False                                     # what the rescue rule makes of row 2
    n_chunks = chunks if chunks is not None else K.m2f_attn_chunks(B, A, NK)
    out = K.m2f_masked_attention(q, k, v, B, Q, NK, A=A, bits=bits, allowed=allowed, chunks=chunks)
    out2 = K.m2f_masked_attention(q, k, v, B, Q, NK, A=A, bits=bits, allowed=allowed, chunks=chunks)
    ws = None
    if n_chunks > 1:
        ws = torch.full((_lib.value("mss_m2f_attn_workspace_bytes", B, Q, A, n_chunks) // 4,), float("nan"), device="cuda")
    out3 = K.m2f_masked_attention(q, k, v, B, Q, NK, A=A, bits=bits, allowed=allowed, chunks=chunks, ws=ws)
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and torch.equal(out, out3)
    ref64 = attention_reference(q, k, v, mask, B, Q, NK, A, torch.float64)
    ref32 = attention_reference(q, k, v, mask, B, Q, NK, A, torch.float32)
    e32 = float((ref32.double() - ref64).abs().max())
    err = float((out.double() - ref64).abs().max())
    print(f"B {B} Q {Q} NK {NK} A {A} chunks {n_chunks} masked {masked}: kernel {err:.3g} torch-fp32 {e32:.3g}")
    assert torch.isfinite(out).all()
    assert err <= 4.0 * e32, (err, e32)


# ---- 5 / 6. the whole decoder ------------------------------------------------------------------------------------------------------
def build_module(seed, **geometry):
    from multishiftseg_amd import MultiScaleMaskedTransformerDecoder_GMA
    geom = dict(GEOM, **geometry)
    m = MultiScaleMaskedTransformerDecoder_GMA(256, True, **geom)
    m.load_state_dict(R.synth_state_dict(seed, num_layers=geom["dec_layers"], num_queries=geom["num_queries"],
                                         enforce_input_project=geom["enforce_input_project"]), strict=True)
    return m.cuda().eval()


def rescued(mask):
    mask = mask.clone()
    mask[torch.where(mask.sum(-1) == mask.shape[-1])] = False
    return mask


def check_against_helper(out, x, feat, seed, tau, near_count, noise_class, noise_masks, Q=100, layers=9):
    """The protocol of the whole-decoder tests. The module's mask bits are forced into the float64 helper (CPU), so module and
    helper walk the same trajectory; then (ii) every module bit that differs from the helper's own float64 threshold of ITS
    interpolated logits sits at |x| < tau, at most near_count[layer] of them, and (iii) every returned tensor is within
    max(1e-5 rms, 4 x noise) of the helper's."""
    forced = []
    for words in out["attn_bits"]:
        m = unpack(words, Q).transpose(2, 3).cpu()                 # [B, 2, Q, HW]
        forced.append((m[:, 0].contiguous(), m[:, 1].contiguous()))
    sd = R.synth_state_dict(seed, dtype=torch.float64, num_layers=layers, num_queries=Q)
    with torch.no_grad():
        ref = R.decoder_forward(sd, [torch.from_numpy(v).double() for v in x], torch.from_numpy(feat).double(), layers,
                                forced_bits=forced, return_interp=True)
    flips = []
    for i, ((fg, bg), it) in enumerate(zip(forced, ref["interp"])):
        it = it.flatten(2)
        want_fg, want_bg = rescued(it < 0), rescued(it > 0)
        d = (fg != want_fg) | (bg != want_bg)
        flips.append(int(d.sum()))
        assert not (d & ~(it.abs() < tau)).any(), f"layer {i}: a mask bit differs where |logit| >= tau = {tau:.3g}"
        assert flips[-1] <= int(near_count[i]), f"layer {i}: {flips[-1]} differing bits, {int(near_count[i])} logits below tau"
    print("differing mask bits per layer:", flips, "logits below tau:", [int(c) for c in near_count])

    def close(name, got, want, noise):
        rms = float(want.pow(2).mean().sqrt())
        err = float((got.detach().double().cpu() - want).abs().max())
        bound = max(1e-5 * rms, 4.0 * noise)
        print(f"{name}: err {err:.3g} bound {bound:.3g} (rms {rms:.3g})")
        assert err <= bound, (name, err, bound)
    for key in ("pred_logits", "pred_logits_ood"):
        close(key, out[key], ref[key], noise_class)
    for key in ("pred_masks", "pred_masks_ood"):
        close(key, out[key], ref[key], noise_masks)
    assert len(out["aux_outputs"]) == len(ref["aux_outputs"]) == layers - 1
    for j, (a, b) in enumerate(zip(out["aux_outputs"], ref["aux_outputs"])):
        for key in ("pred_logits", "pred_logits_ood"):
            close(f"aux{j}.{key}", a[key], b[key], noise_class)
        for key in ("pred_masks", "pred_masks_ood"):
            close(f"aux{j}.{key}", a[key], b[key], noise_masks)
    assert out["pred_masks_ood"] is out["pred_masks"]
    return ref


def test_whole_decoder_against_the_reference_fixture(gemm_route):
    fix = golden("m2f_transformer_decoder")
    sizes = [tuple(int(v) for v in s) for s in fix["sizes"]]
    x, feat = R.synth_inputs(int(fix["input_seed"]), 2, sizes[:3], sizes[3])
    m = build_module(int(fix["seed"]))
    with torch.no_grad():
        out = m([torch.from_numpy(v).cuda() for v in x], torch.from_numpy(feat).cuda(), return_attn_bits=True)
    ref = check_against_helper(out, x, feat, int(fix["seed"]), float(fix["tau"]), fix["near_count"], float(fix["noise_class"]),
                               float(fix["noise_masks"]))
    # the stored outputs of the reference itself, on top of the helper's: final logits within the same bound + the helper's own distance
    for key, noise in (("pred_logits", "noise_class"), ("pred_logits_ood", "noise_class")):
        err = float(np.abs(out[key].cpu().double().numpy() - fix[key]).max())
        assert err <= 8.0 * float(fix[noise]), (key, err)
    assert float((ref["pred_logits"] - torch.from_numpy(fix["pred_logits"]).double()).abs().max()) <= 2.0 * float(fix["noise_class"])


REAL_SIZES = {"704": (2, [(22, 22), (44, 44), (88, 88)], (176, 176)), "1024x2048": (1, [(32, 64), (64, 128), (128, 256)], (256, 512))}


@pytest.mark.parametrize("name", list(REAL_SIZES))
def test_whole_decoder_at_real_sizes(name, gemm_route):
    """Same protocol as the fixture test with the helper as the reference: noise_* = max |fp32 - fp64| of the helper under the
    same forced bits (all prediction steps), tau = 8 x noise_masks, the per-layer count from the float64 run."""
    B, sizes, fsize = REAL_SIZES[name]
    seed = 21
    x, feat = R.synth_inputs(211, B, sizes, fsize)
    m = build_module(seed)
    with torch.no_grad():
        out = m([torch.from_numpy(v).cuda() for v in x], torch.from_numpy(feat).cuda(), return_attn_bits=True)
    forced = []
    for words in out["attn_bits"]:
        mk = unpack(words, 100).transpose(2, 3).cpu()
        forced.append((mk[:, 0].contiguous(), mk[:, 1].contiguous()))
    runs = {}
    for dtype in (torch.float32, torch.float64):
        sd = R.synth_state_dict(seed, dtype=dtype)
        with torch.no_grad():
            runs[dtype] = R.decoder_forward(sd, [torch.from_numpy(v).to(dtype) for v in x], torch.from_numpy(feat).to(dtype), 9,
                                            forced_bits=forced, return_interp=True)
    r32, r64 = runs[torch.float32], runs[torch.float64]
    dmax = lambda a, b: max(float((p.double() - q).abs().max()) for p, q in zip(a, b))
    noise_class = max(dmax(r32["all_logits"], r64["all_logits"]), dmax(r32["all_logits_ood"], r64["all_logits_ood"]))
    noise_masks = dmax(r32["all_masks"], r64["all_masks"])
    tau = 8.0 * noise_masks
    near = [int((t.abs() < tau).sum()) for t in r64["interp"]]
    print(f"{name}: noise class {noise_class:.3g} masks {noise_masks:.3g} tau {tau:.3g}")
    del runs, r32, r64
    check_against_helper(out, x, feat, seed, tau, near, noise_class, noise_masks)


def test_small_query_count_and_input_projection(gemm_route):
    """37 queries (not a multiple of 32 or 4), 2 layers, the 1x1 input projection: against the float64 helper under forced bits,
    with the helper's own fp32-vs-fp64 distance as the noise."""
    B, sizes, fsize, Q, L, seed = 2, [(3, 5), (6, 10), (12, 20)], (24, 40), 37, 2, 33
    x, feat = R.synth_inputs(331, B, sizes, fsize)
    m = build_module(seed, num_queries=Q, dec_layers=L, enforce_input_project=True)
    sd_names = dict(num_layers=L, num_queries=Q, enforce_input_project=True)
    with torch.no_grad():
        out = m([torch.from_numpy(v).cuda() for v in x], torch.from_numpy(feat).cuda(), return_attn_bits=True)
    forced = []
    for words in out["attn_bits"]:
        mk = unpack(words, Q).transpose(2, 3).cpu()
        forced.append((mk[:, 0].contiguous(), mk[:, 1].contiguous()))
    runs = {}
    for dtype in (torch.float32, torch.float64):
        with torch.no_grad():
            runs[dtype] = R.decoder_forward(R.synth_state_dict(seed, dtype=dtype, **sd_names), [torch.from_numpy(v).to(dtype) for v in x],
                                            torch.from_numpy(feat).to(dtype), L, forced_bits=forced, return_interp=True)
    r32, r64 = runs[torch.float32], runs[torch.float64]
    dmax = lambda a, b: max(float((p.double() - q).abs().max()) for p, q in zip(a, b))
    noise_masks = dmax(r32["all_masks"], r64["all_masks"])
    tau = 8.0 * noise_masks
    for i, ((fg, bg), it) in enumerate(zip(forced, r64["interp"])):
        it = it.flatten(2)
        d = (fg != rescued(it < 0)) | (bg != rescued(it > 0))
        assert not (d & ~(it.abs() < tau)).any() and int(d.sum()) <= int((it.abs() < tau).sum()), i
    for key, noise in (("pred_logits", dmax(r32["all_logits"], r64["all_logits"])), ("pred_logits_ood", dmax(r32["all_logits_ood"], r64["all_logits_ood"])),
                       ("pred_masks", noise_masks)):
        want = r64[key]
        err = float((out[key].double().cpu() - want).abs().max())
        bound = max(1e-5 * float(want.pow(2).mean().sqrt()), 4.0 * noise)
        print(f"{key}: err {err:.3g} bound {bound:.3g}")
        assert err <= bound, (key, err, bound)
    assert len(out["aux_outputs"]) == L - 1


# ---- 7. the fused score ----------------------------------------------------------------------------------------------------------
def test_fuse_score_equals_the_score_kernel_on_the_returned_outputs(gemm_route):
    from multishiftseg_amd import kernels as K
    fix = golden("m2f_transformer_decoder")
    sizes = [tuple(int(v) for v in s) for s in fix["sizes"]]
    x, feat = R.synth_inputs(int(fix["input_seed"]), 2, sizes[:3], sizes[3])
    m = build_module(int(fix["seed"]))
    xs, ft = [torch.from_numpy(v).cuda() for v in x], torch.from_numpy(feat).cuda()
    with torch.no_grad():
        plain = m(xs, ft)
        fused = m(xs, ft, fuse_score=(96, 160))
    assert fused["pred_masks"] is None and fused["pred_masks_ood"] is None and "ood_score" not in plain
    assert torch.equal(plain["pred_logits_ood"], fused["pred_logits_ood"]) and torch.equal(plain["pred_logits"], fused["pred_logits"])
    want = K.m2f_score_fused(plain["pred_logits_ood"], plain["pred_masks_ood"].permute(0, 2, 3, 1).contiguous(), (96, 160))
    assert fused["ood_score"].shape == (2, 96, 160) and torch.equal(fused["ood_score"], want)
    assert torch.isfinite(want).all()


# ---- 8. dirty scratch --------------------------------------------------------------------------------------------------------------
def test_whole_module_on_poisoned_scratch():
    fix = golden("m2f_transformer_decoder")
    sizes = [tuple(int(v) for v in s) for s in fix["sizes"]]
    x, feat = R.synth_inputs(int(fix["input_seed"]), 2, sizes[:3], sizes[3])
    m = build_module(int(fix["seed"]))
    xs, ft = [torch.from_numpy(v).cuda() for v in x], torch.from_numpy(feat).cuda()

    def fn():
        with torch.no_grad():
            out = m(xs, ft, fuse_score=(96, 160), return_attn_bits=True)
        return {"logits": out["pred_logits"], "ood": out["pred_logits_ood"], "score": out["ood_score"], "bits": out["attn_bits"],
                "aux": [a["pred_masks"] for a in out["aux_outputs"]]}
    runs = poison.poison_runs(fn, bitwise=True)
    assert all(runs["reproducible"])


# ---- stage 1: the only gradient ------------------------------------------------------------------------------------------------------
def test_stage1_gradient_reaches_class_embed2_only(gemm_route):
    fix = golden("m2f_transformer_decoder")
    sizes = [tuple(int(v) for v in s) for s in fix["sizes"]]
    x, feat = R.synth_inputs(int(fix["input_seed"]), 2, sizes[:3], sizes[3])
    m = build_module(int(fix["seed"]))
    xs, ft = [torch.from_numpy(v).cuda() for v in x], torch.from_numpy(feat).cuda()
    with pytest.raises(NotImplementedError):
        m(xs, ft)                                                      # every parameter trainable: not a supported mode
    for p in m.parameters():
        p.requires_grad_(False)
    m.class_embed2.weight.requires_grad_(True)
    m.class_embed2.bias.requires_grad_(True)
    out = m(xs, ft)
    cot = torch.randn(out["pred_logits_ood"].shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    (out["pred_logits_ood"] * cot).sum().backward()
    assert not out["pred_logits"].requires_grad and not out["pred_masks"].requires_grad
    # against autograd through the float64 helper. Bound: the gradient is cot^T dn over 200 rows, dn = decoder_norm(final state) of
    # rms 1 carrying the decoder's fp32 noise (noise_masks / mask rms ~ 6e-6 relative); the 200-term fp32 sums add <= 200 * 2^-24 =
    # 1.2e-5: 1e-4 relative L2 leaves a factor of five.
    ref_sd = R.synth_state_dict(int(fix["seed"]), dtype=torch.float64)
    ref_sd["class_embed2.weight"].requires_grad_(True)
    ref_sd["class_embed2.bias"].requires_grad_(True)
    ref = R.decoder_forward(ref_sd, [torch.from_numpy(v).double() for v in x], torch.from_numpy(feat).double(), 9)
    (ref["pred_logits_ood"] * cot.cpu().double()).sum().backward()
    for name in ("weight", "bias"):
        got, want = getattr(m.class_embed2, name).grad.cpu().double(), ref_sd["class_embed2." + name].grad
        rel = float((got - want).norm() / want.norm())
        print(f"class_embed2.{name}.grad rel L2 {rel:.3g}")
        assert rel <= 1e-4, (name, rel)
