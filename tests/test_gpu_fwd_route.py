"""One small call per class of csrc/fwd_route.h -- (kernel, tile width, loader variant, MFMA shape) -- that default switches can reach,
at the smallest shape that reaches it: mss_conv2d_forward_route must answer the class's code, the output must match a float64
reference within the bound tests/test_gpu_ops.py applies to that route (allowed_error below), and the native fp32 routes must be
bit-identical under MSS_GEMM_VARIANT=2 + MSS_GEMM_TAIL=0 (variant 3 and the hybrid change the schedule only). tools/fwd_route_parity.py runs the same table against another build of the library.

Which class a row lands in is checked on the host for the same rules (tests/test_fwd_route_cpu.py); here the class is in the name."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# name: (code, kind, params). kinds: "gemm" rows / C / K over `batch` entries; "conv" an R x R convolution; "dgrad" stride -2; "stem"
CASES = {
    "igemm_256x64": (0, "conv", dict(N=1, H=20, W=24, C=32, K=48, R=3)),
    "igemm_128x128x16": (0, "conv", dict(N=2, H=13, W=17, C=32, K=200, R=3, affine=True)),
    "igemm_128x128x32": (0, "conv", dict(N=1, H=9, W=11, C=2048, K=128, R=3, dil=2)),
    "igemm_per_sample": (0, "conv", dict(N=3, H=9, W=11, C=32, K=128, R=3, affine=True, per_sample=True)),
    "igemm_1x1_stride2": (0, "conv", dict(N=1, H=21, W=19, C=64, K=128, R=1, stride=2)),
    "igemm_bn64_below_16384_rows": (0, "gemm", dict(rows=16383, C=64, K=48)),
    "dgrad_s2_256x64": (6, "dgrad", dict(N=1, H=9, W=7, C=32, K=48, R=3)),
    "dgrad_s2_128x128": (6, "dgrad", dict(N=2, H=6, W=9, C=64, K=200, R=1)),
    "stem7": (5, "stem", dict(N=2, H=37, W=51)),
    "few_rows_8": (2, "gemm", dict(rows=5, C=528, K=100)),
    "few_rows_16": (2, "gemm", dict(rows=9, C=64, K=19)),
    "few_rows_32": (2, "gemm", dict(rows=32, C=512, K=48)),
    "gemm_nt_bn64_v3": (1, "gemm", dict(rows=16384, C=64, K=48)),
    "gemm_nt_bn128_v3": (1, "gemm", dict(rows=300, C=64, K=136, affine=True)),
    "gemm_nt_bn128_v2": (1, "gemm", dict(rows=300, C=32, K=128)),                      # two K-steps per tile: variant 2 by shape
    "gemm_nt_bn128_v3_batched": (1, "gemm", dict(rows=257, C=48, K=128, batch=3)),
    "gemm_nt_bn256_wide_v3": (1, "gemm", dict(rows=131072, C=256, K=256)),              # 1024 wide tiles: two rounds
    "gemm_nt_bn256_hybrid_v3": (1, "gemm", dict(rows=32896, C=256, K=512)),             # 514 wide tiles = 512 + 2 -> 4 narrow
    "gemm_nt_per_sample_whole_tiles": (1, "gemm", dict(rows=3 * 256, C=64, K=128, affine=True, per_sample=3)),
    "perimg_bn128": (1, "gemm", dict(rows=3 * 128, C=128, K=128, per_image=3)),
    "perimg_bn256": (1, "gemm", dict(rows=2 * 65536, C=256, K=256, per_image=2)),       # 1024 wide tiles
    "k_imgs_bn128": (1, "gemm", dict(rows=200, C=96, K=128, batch=4, k_imgs=2)),
    "k_imgs_bn256": (1, "gemm", dict(rows=16384, C=256, K=256, batch=8, k_imgs=2)),     # 8 x 128 x 1 = 1024 wide tiles
    "split_bn128_mfma16": (3, "gemm", dict(rows=300, C=64, K=136, split=True)),
    "split_bn128_mfma32": (3, "gemm", dict(rows=300, C=64, K=136, split=True, affine=True)),
    "split_bn256_mfma16": (3, "gemm", dict(rows=131072, C=256, K=256, split=True)),
    "split_bn256_mfma32": (3, "gemm", dict(rows=131072, C=256, K=256, split=True, affine=True)),
    "split_conv_bn128": (4, "conv", dict(N=2, H=13, W=17, C=32, K=200, R=3, affine=True, split=True)),
    "split_conv_bn256": (4, "conv", dict(N=1, H=256, W=512, C=16, K=256, R=3, split=True)),   # 1024 wide tiles
    "split_rowaff": (4, "gemm", dict(rows=3 * 100, C=64, K=128, split=True, affine=True, per_sample=3)),
}
NATIVE = [n for n, (code, _, p) in CASES.items() if not p.get("split")]


def allowed_error(code, ref, mag, terms):
    """Elementwise bound on |y - ref| per route code, as tests/test_gpu_ops.py has it for that route:
    0 (conv_igemm_kernel): test_conv_vs_oracle's rtol = atol = 1e-4 on outputs of unit scale (weights scaled by 1 / sqrt(fan-in), as here);
    1, 3, 4 (the NT GEMM kernels and both split forms): 2e-6 of max |y| (test_bf16x3_gemm_is_fp32_accurate, test_bf16x3_implicit_gemm_vs_float64);
    2 (few rows): 1e-5 * max(1, max |y|) (test_few_rows_1x1_route).
    5, 6 (stem, stride-2 data gradient; not in that file): the forward bound of tests/test_gpu_stem7.py -- twice the first-order bound
    of an fp32 chain of `terms` fused multiply-adds, terms * 2^-24 * sum |x| |w| (`mag`), plus one rounding of the result."""
    top = ref.abs().max().item()
    if code == 0:
        return 1e-4 + 1e-4 * ref.abs()
    if code == 2:
        return torch.full_like(ref, 1e-5 * max(1.0, top))
    if code in (5, 6):
        return 2 * (terms + 3) * 2.0 ** -24 * mag + 2.0 ** -23 * ref.abs()
    return torch.full_like(ref, 2e-6 * top)


def build(name):
    """(MssConvArgs, output tensor, (float64 reference, the view of the output it covers, sum |x| |w| where allowed_error wants it,
    terms per output), tensors to keep alive)"""
    from multishiftseg_amd import _lib, kernels as K
    from multishiftseg_amd._lib import MssConvArgs, ptr
    code, kind, p = CASES[name]
    g = torch.Generator(device="cuda").manual_seed(sum(map(ord, name)))

    def randn(*shape):
        return torch.randn(*shape, device="cuda", generator=g)

    a = MssConvArgs()
    keep = []
    if kind == "gemm":
        rows, C, Ko, batch = p["rows"], p["C"], p["K"], p.get("batch", 1)
        kpad = _lib.value("mss_conv2d_kpad", Ko)
        imgs = p.get("per_image") or p.get("per_sample") or 1
        x = randn(batch, rows, C)
        nw = imgs if p.get("per_image") else batch                      # weight sets: per image (one-batch form) or per batch entry
        w = torch.zeros(nw, kpad, C, device="cuda")
        w[:, :Ko] = randn(nw, Ko, C) / C ** 0.5
        y = torch.full((batch, rows, Ko), float("nan"), device="cuda")
        a.N, a.H, a.W = imgs, 1, rows // imgs
        a.OH, a.OW = a.H, a.W
        a.R = a.S = a.stride = a.dil = 1
        xin = x.double()
        if p.get("affine"):
            ns = p.get("per_sample", 1)
            sc, sh = torch.rand(ns, C, device="cuda", generator=g) + 0.5, randn(ns, C) * 0.3
            a.in_scale, a.in_shift, a.in_relu, a.in_ss_stride = ptr(sc), ptr(sh), 1, C if p.get("per_sample") else 0
            per_row = torch.arange(rows, device="cuda") // (rows // ns)
            xin = torch.relu(xin * sc.double()[per_row] + sh.double()[per_row])
            keep += [sc, sh]
        wd = w[:, :Ko].double()
        if p.get("per_image") or p.get("k_imgs"):
            n_img = p.get("per_image") or p["k_imgs"]
            steps = torch.tensor([3 + (2 * i) % (C // 16 - 3 + 1) for i in range(n_img)], dtype=torch.int32)
            ksteps = steps.cuda()
            keep.append(ksteps)
            a.k_steps = ptr(ksteps)
            if p.get("k_imgs"):
                a.k_imgs, a.k_base = p["k_imgs"], 1
                used = [16 * (1 + int(steps[b % n_img])) for b in range(batch)]        # k_base + k_steps[image] K-steps
                assert max(used) <= C
                col = torch.arange(C, device="cuda")
                mask = torch.stack([(col < u) for u in used]).double()               # [batch][C]
                xin = xin * mask[:, None, :]
            else:
                a.w_img_stride = kpad * C
                col = torch.arange(C, device="cuda")
                mask = torch.stack([(col < 16 * int(s)) for s in steps]).double()    # [imgs][C]
                per_row = torch.arange(rows, device="cuda") // (rows // n_img)
                xin = xin * mask[per_row][None]
        sel = torch.randint(0, rows, (min(rows, 2048),), device="cuda", generator=g) if rows > 4096 else torch.arange(rows, device="cuda")
        if p.get("per_image"):                                           # image i's rows on its own weights
            sel = sel.sort().values
            per_row = sel // (rows // imgs)
            ref = torch.cat([torch.einsum("bmc,kc->bmk", xin[:, sel[per_row == i]], wd[i]) for i in range(imgs)], dim=1)
        else:
            ref = torch.einsum("bmc,bkc->bmk", xin[:, sel], wd)
        a.x, a.w, a.y = ptr(x), ptr(w), ptr(y)
        a.C, a.ldx, a.K, a.Kpad, a.ldy = C, C, Ko, kpad, Ko
        if batch > 1:
            a.batch, a.x_bs, a.w_bs, a.y_bs = batch, rows * C, kpad * C, rows * Ko
        if p.get("split"):
            planes = K.split_planes(w, kpad, C)
            a.w_split = ptr(planes)
            keep.append(planes)
        keep += [x, w]
        return a, y, (ref, lambda t: t[:, sel], None, C), keep
    if kind == "stem":
        img, wt = randn(p["N"], 3, p["H"], p["W"]), randn(64, 3, 7, 7) / 12
        x, pw = K.image_to_nhwc(img, Cp=4), K.packed_stem7(wt)
        OH, OW = (p["H"] - 1) // 2 + 1, (p["W"] - 1) // 2 + 1
        y = torch.full((p["N"], OH, OW, 64), float("nan"), device="cuda")
        a = K._conv_args(x, pw, None, 2, 1, 3, None, False, None, False, None)
        a.y, a.OH, a.OW, a.ldy = ptr(y), OH, OW, 64
        ref = F.conv2d(img.double(), wt.double(), stride=2, padding=3).permute(0, 2, 3, 1)
        mag = F.conv2d(img.double().abs(), wt.double().abs(), stride=2, padding=3).permute(0, 2, 3, 1)
        return a, y, (ref, lambda t: t, mag, 147), [x, pw, img, wt]
    N, H, W, C, Ko, R = (p[k] for k in "NHWCKR")
    stride, dil = p.get("stride", 1), p.get("dil", 1)
    pad = dil * (R // 2)
    x = K.Act(randn(N, H, W, C))
    xin = x.buf.double()
    aff = mag = None
    if p.get("affine"):
        ns = N if p.get("per_sample") else 1
        sc, sh = torch.rand(ns, C, device="cuda", generator=g) + 0.5, randn(ns, C) * 0.3
        aff = (sc, sh) if p.get("per_sample") else (sc[0].contiguous(), sh[0].contiguous())
        xin = torch.relu(xin * sc.double().view(ns, 1, 1, C) + sh.double().view(ns, 1, 1, C))
    if kind == "dgrad":
        wt = randn(C, Ko, R, R) / (C * R * R) ** 0.5                     # the strided forward's weight: Ko -> C channels
        pw = K.pack_weight(wt, flip=True)
        OH, OW = 2 * H - (1 if R == 3 else 0), 2 * W
        a = K._conv_args(x, pw, None, -2, 1, pad, aff, aff is not None, None, False, None)
        op = (OH - ((H - 1) * 2 - 2 * pad + R), OW - ((W - 1) * 2 - 2 * pad + R))
        ref = F.conv_transpose2d(xin.permute(0, 3, 1, 2), wt.double(), stride=2, padding=pad, output_padding=op).permute(0, 2, 3, 1)
        mag = F.conv_transpose2d(xin.permute(0, 3, 1, 2).abs(), wt.double().abs(), stride=2, padding=pad, output_padding=op).permute(0, 2, 3, 1)
    else:
        wt = randn(Ko, C, R, R) / (C * R * R) ** 0.5
        K.set_gemm_route("bf16x3" if p.get("split") else "native")
        try:
            pw = K.pack_weight(wt)
            a = K._conv_args(x, pw, None, stride, dil, pad, aff, aff is not None, None, False, None)
        finally:
            K.set_gemm_route(None)
        OH, OW = K.conv_out_size(H, R, stride, dil, pad), K.conv_out_size(W, R, stride, dil, pad)
        ref = F.conv2d(xin.permute(0, 3, 1, 2), wt.double(), stride=stride, dilation=dil, padding=pad).permute(0, 2, 3, 1)
    y = torch.full((N, OH, OW, Ko), float("nan"), device="cuda")
    a.y, a.OH, a.OW, a.ldy = ptr(y), OH, OW, Ko
    return a, y, (ref, lambda t: t, mag, C * R * R), [x, pw, wt, aff]


def launch(name, env=None):
    """the case under `env` (switches of the library): (route code, output, (reference, view of the output it covers))"""
    from multishiftseg_amd import _lib
    env = env or {}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    _lib.reset_env_cache()
    try:
        a, y, ref, keep = build(name)
        code = _lib.value("mss_conv2d_forward_route", ctypes.byref(a))
        _lib.call("mss_conv2d_forward_f32", ctypes.byref(a))
        torch.cuda.synchronize()
        mf = _lib.value("mss_gemm_split_last_mfma")
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        _lib.reset_env_cache()
    return code, y, ref, mf


@pytest.mark.parametrize("name", list(CASES))
def test_class_gets_its_code_and_matches_float64(name):
    code, y, (ref, view, mag, terms), mf = launch(name)
    assert code == CASES[name][0]
    assert torch.isfinite(y).all() and ref.shape == view(y).shape and ref.abs().max().item() > 0.1
    err = (view(y).double() - ref).abs()
    worst = (err / allowed_error(code, ref, mag, terms).clamp_min(1e-300)).max().item()     # (an output without a live tap: 0 of 0 allowed)
    print(f"{name}: max |err| / max |y| = {err.max().item() / ref.abs().max().item():.3g}, max |err| / allowed = {worst:.3g}")
    assert worst <= 1.0
    if "mfma" in name:
        assert mf == int(name[-2:])


@pytest.mark.parametrize("name", NATIVE)
def test_native_routes_are_bitwise_variant_2_without_the_hybrid(name):
    _, y, _, _ = launch(name)
    code, y2, _, _ = launch(name, {"MSS_GEMM_VARIANT": "2", "MSS_GEMM_TAIL": "0"})
    assert code == CASES[name][0] and torch.equal(y, y2)
