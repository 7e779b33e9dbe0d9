"""The kernels of the dropped-channel ASPP products alone: the two-source input transform that writes image n's
columns [u ; kept channels of v] only (mss_wino_input_transform_aspp3_dropped_f32), the per-image weight forms, the (position, image)
batch entries of gemm_nt_kernel's per-image mode, the per-image form of gemm_tn_direct_kernel and the column gather that brings
the weight gradients back to channel order. NaN stands behind every buffer and in every column that must be neither written nor read."""
import ctypes

import pytest
import torch

from multishiftseg_amd import _lib, kernels as K
from multishiftseg_amd._lib import MssConvArgs, call, ptr, status

pytestmark = pytest.mark.gpu

CANARY = 64
NAN = float("nan")


def _off(t, floats):
    return ctypes.c_void_p(t.data_ptr() + 4 * floats)


def _with_canary(n):
    return torch.full((n + CANARY,), NAN, device="cuda", dtype=torch.float32)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _mask(mode, n, C1, g):
    """[n][C1] of {0, 2}: the Dropout2d keep mask (p = 0.5) with the edge the mode names in image 0."""
    keep = torch.rand((n, C1), device="cuda", generator=g) >= 0.5
    if mode == "all":
        keep[0] = True
    elif mode == "none":
        keep[0] = False                                   # k_steps floor: 3 steps = 48 zero columns
    elif mode == "mod16":
        keep[0] = False
        keep[0, torch.randperm(C1, device="cuda", generator=g)[:17]] = True        # kept count = 1 mod 16
    elif mode == "common":
        keep[:, 5] = False                                # a channel no image keeps
    return keep.float() * 2.0


# (n, H, W, C0, C1, d, tiles): 1 x 2-pixel sub-grids; a 32-channel chunk that straddles the two sources (48 = 32 + 16); more chunks in
# source 0 than in source 1
TRANSFORM_CASES = [(2, 12, 16, 32, 64, 12, (4, 4, 4)), (3, 45, 75, 48, 80, 6, (6, 4, 6)), (2, 24, 36, 128, 64, 2, (4, 6, 4))]


@pytest.mark.parametrize("mode", ["random", "all", "none", "mod16", "common"])
@pytest.mark.parametrize("n,H,W,C0,C1,d,tiles", TRANSFORM_CASES)
def test_dropped_transform_writes_the_dense_columns_of_the_kept_channels(n, H, W, C0, C1, d, tiles, mode):
    g = torch.Generator(device="cuda").manual_seed(1000 * H + W + C0 + len(mode))
    C = C0 + C1
    ld0, ld1, o0, o1 = C0 + 8, C1 + 12, 4, 8
    b0 = torch.randn((n, H, W, ld0), device="cuda", generator=g)
    b1 = torch.randn((n, H, W, ld1), device="cuda", generator=g)
    a0, a1 = _off(b0, o0), _off(b1, o1)
    sc0 = torch.randn(C0, device="cuda", generator=g)
    sh0 = torch.rand(C0, device="cuda", generator=g) + 0.25
    mask = _mask(mode, n, C1, g)
    sc1 = (torch.randn(C1, device="cuda", generator=g)[None] * mask).contiguous()
    sh1 = ((torch.rand(C1, device="cuda", generator=g) + 0.25)[None] * mask).contiguous()
    ctiles = (ctypes.c_int * 3)(*tiles)
    Ts = [_lib.value("mss_wino_num_tiles", n, H, W, (m + 1) * d, t) for m, t in enumerate(tiles)]
    Ps = [(t + 2) ** 2 for t in tiles]
    sizes = [p * T * C for p, T in zip(Ps, Ts)]

    # the dense two-source transform: the second formulation
    want = [_with_canary(s) for s in sizes]
    sums0, gap0 = _with_canary(n * d * d * C), _with_canary(n * C)
    rc = status("mss_wino_input_transform_aspp3_src2_f32", a0, ld0, C0, ptr(sc0), ptr(sh0), 0, a1, ld1, C1, ptr(sc1), ptr(sh1), C1,
                n, H, W, d, ctiles, *[ptr(t) for t in want], ptr(sums0), ptr(gap0))
    assert rc == 0, rc

    _idx, count, k_steps, place, col = K.chan_compact_index(mask, want_col=True)
    xc = _with_canary(n * H * W * C1)                       # columns behind 16 * k_steps[n] stay NaN: the transform must not read them
    call("mss_chan_compact_act_f32", a1, ld1, ptr(xc), C1, n, H * W, C1, ptr(place), ptr(k_steps), ptr(sc1), ptr(sh1))
    got = [_with_canary(s) for s in sizes]
    sums, gap = _with_canary(n * d * d * C), _with_canary(n * C)
    rc = status("mss_wino_input_transform_aspp3_dropped_f32", a0, ld0, C0, ptr(sc0), ptr(sh0), 0, ptr(xc), C1, C1, ptr(place), ptr(k_steps),
                n, H, W, d, ctiles, *[ptr(t) for t in got], ptr(sums), ptr(gap))
    assert rc == 0, rc
    ks, cnt, pl = k_steps.cpu().tolist(), count.cpu().tolist(), place.cpu()
    assert all(k == max(3, -(-c // 16)) for k, c in zip(ks, cnt))
    if mode == "none":
        assert cnt[0] == 0 and ks[0] == 3
    if mode == "mod16":
        assert cnt[0] % 16 == 1
    for m in range(3):
        P, T = Ps[m], Ts[m]
        Ti = T // n
        assert T % n == 0
        w = want[m][:sizes[m]].view(P, T, C)
        o = got[m][:sizes[m]].view(P, T, C)
        assert not torch.isnan(w).any()
        assert torch.isnan(got[m][sizes[m]:]).all()
        for i in range(n):
            ext = 16 * ks[i]
            rows = slice(i * Ti, (i + 1) * Ti)
            assert torch.equal(_bits(o[:, rows, :C0]), _bits(w[:, rows, :C0])), (m, i, "first factor")
            p_i = pl[i, :ext].cuda().long()
            exp = torch.where((p_i >= 0)[None, None, :], w[:, rows, C0:][:, :, p_i.clamp_min(0)], torch.zeros((), device="cuda"))
            assert torch.equal(_bits(o[:, rows, C0:C0 + ext]), _bits(exp)), (m, i, "compacted columns")
            assert torch.isnan(o[:, rows, C0 + ext:]).all(), (m, i, "behind the extent")
    assert torch.equal(_bits(sums[:n * d * d * C]), _bits(sums0[:n * d * d * C])) and torch.equal(_bits(gap[:n * C]), _bits(gap0[:n * C]))
    assert torch.isnan(sums[n * d * d * C:]).all() and torch.isnan(gap[n * C:]).all()
    dropped = (mask == 0)
    assert float(gap[:n * C].view(n, C)[:, C0:][dropped].abs().max() if dropped.any() else 0.0) == 0.0


def _dropped_state(mask, C0):
    """An AsppDropped without its activation pass (the product tests bring their own X')."""
    d = K.AsppDropped.__new__(K.AsppDropped)
    d.N, d.C0, d.C1 = mask.shape[0], C0, mask.shape[1]
    _idx, d.count, d.k_steps, d.place, d.col = K.chan_compact_index(mask, want_col=True)
    d.xc = None
    return d


def _operands(P, n, Ti, C0, C1, Kout, seed):
    """Dense X' [P][n Ti][C] whose dropped channels are exact zeros per image, dY' [P][n Ti][K], the mask and the compacted X' (NaN
    behind every image's extent), gathered here with torch: independent of the kernels under test."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    C = C0 + C1
    mask = _mask("common", n, C1, g)
    xt = torch.randn((P, n * Ti, C), device="cuda", generator=g)
    dyt = torch.randn((P, n * Ti, Kout), device="cuda", generator=g)
    drop = _dropped_state(mask, C0)
    ks, pl = drop.k_steps.cpu().tolist(), drop.place.cpu()
    xc = torch.full((P, n * Ti, C), NAN, device="cuda")
    for i in range(n):
        rows = slice(i * Ti, (i + 1) * Ti)
        xt[:, rows, C0:] *= (mask[i] != 0).float()[None, None, :]
        ext = 16 * ks[i]
        p_i = pl[i, :ext].cuda().long()
        xc[:, rows, :C0] = xt[:, rows, :C0]
        xc[:, rows, C0:C0 + ext] = torch.where((p_i >= 0)[None, None, :], xt[:, rows, C0:][:, :, p_i.clamp_min(0)], torch.zeros((), device="cuda"))
    return mask, drop, xt, xc, dyt, ks, pl


def _forward_args(x, w, y, batch, rows, C, Kout, w_bs):
    a = MssConvArgs()
    a.x, a.w, a.y = ptr(x), ptr(w), ptr(y)
    a.N, a.H, a.W, a.C, a.ldx = 1, 1, rows, C, C
    a.OH, a.OW, a.K, a.Kpad, a.ldy = 1, rows, Kout, Kout, Kout
    a.R, a.S, a.stride, a.dil, a.pad = 1, 1, 1, 1, 0
    a.batch, a.x_bs, a.w_bs, a.y_bs = batch, rows * C, w_bs, rows * Kout
    return a


# (P, n, tiles per image, C0, C1, K): 200 rows per entry = one whole and one partial row tile; C = 256 is what the weight gradient's
# 128-column tiles ask for; the last case has 2 x 9 x 128 = 2304 wide tiles (0.9 of five rounds of 512 slots), which the tile rule
# gives the 256-wide kernel (K = 256 there would be 1152 wide tiles = 0.75 of three rounds, and the rule prefers the narrow tile)
PRODUCT_CASES = [(36, 2, 200, 128, 128, 128), (36, 3, 200, 128, 128, 256), (36, 2, 200, 64, 192, 256), (64, 2, 1152, 128, 128, 512)]


@pytest.mark.parametrize("P,n,Ti,C0,C1,Kout", PRODUCT_CASES)
def test_per_image_entries_give_the_dense_products_bits(P, n, Ti, C0, C1, Kout):
    C = C0 + C1
    mask, drop, xt, xc, _dyt, ks, pl = _operands(P, n, Ti, C0, C1, Kout, 7 * P + n + Kout)
    g = torch.Generator(device="cuda").manual_seed(Kout + n)
    u = torch.randn((P, Kout, C), device="cuda", generator=g)
    un = torch.full((P, n, Kout, C), NAN, device="cuda")              # U'_n [P][N][K][C]: NaN behind every image's extent
    for i in range(n):
        ext = 16 * ks[i]
        p_i = pl[i, :ext].cuda().long()
        un[:, i, :, :C0] = u[:, :, :C0]
        un[:, i, :, C0:C0 + ext] = torch.where((p_i >= 0)[None, None, :], u[:, :, C0:][:, :, p_i.clamp_min(0)], torch.zeros((), device="cuda"))
    T = n * Ti
    y0, y1 = _with_canary(P * T * Kout), _with_canary(P * T * Kout)
    call("mss_conv2d_forward_f32", ctypes.byref(_forward_args(xt, u, y0, P, T, C, Kout, Kout * C)))
    a = _forward_args(xc, un, y1, P * n, Ti, C, Kout, Kout * C)
    a.k_steps, a.k_base, a.k_imgs = ptr(drop.k_steps), C0 // 16, n
    call("mss_conv2d_forward_f32", ctypes.byref(a))
    assert not torch.isnan(y0[:P * T * Kout]).any()
    assert torch.equal(_bits(y1[:P * T * Kout]), _bits(y0[:P * T * Kout]))
    assert torch.isnan(y1[P * T * Kout:]).all() and torch.isnan(y0[P * T * Kout:]).all()


def test_per_image_weight_forms_are_the_dense_filter_transform_gathered():
    n, C0, C1, Kout, tile = 3, 64, 192, 128, 4
    C, P = C0 + C1, 36
    g = torch.Generator(device="cuda").manual_seed(11)
    mask = _mask("none", n, C1, g)
    drop = _dropped_state(mask, C0)
    w = torch.randn((Kout, C, 3, 3), device="cuda", generator=g)
    pw = K.pack_weight(w)                                    # tap-major rows [9][Kpad][C], as the compose GEMM leaves them
    u = torch.empty((P, Kout, C), device="cuda")
    call("mss_wino_pack_weights_f32", ptr(w), ptr(u), Kout, C, Kout, C, tile)
    ww = K.aspp_dropped_weights(pw.t, Kout, C, pw.Kpad, pw.Cp, tile, drop)
    un = ww.t.view(P, n, Kout, C)
    ks, pl = drop.k_steps.cpu().tolist(), drop.place.cpu()
    for i in range(n):
        ext = 16 * ks[i]
        p_i = pl[i, :ext].cuda().long()
        assert torch.equal(_bits(un[:, i, :, :C0]), _bits(u[:, :, :C0]))
        exp = torch.where((p_i >= 0)[None, None, :], u[:, :, C0:][:, :, p_i.clamp_min(0)], torch.zeros((), device="cuda"))
        assert torch.equal(_bits(un[:, i, :, C0:C0 + ext]), _bits(exp))
        assert float(un[:, i, :, C0 + ext:].abs().max()) == 0.0


def _rel_l2(a, ref):
    return float((a.double().cpu() - ref).norm() / ref.norm())


@pytest.mark.parametrize("P,n,Ti,C0,C1,Kout", PRODUCT_CASES)
def test_per_image_weight_gradient_against_float64(P, n, Ti, C0, C1, Kout):
    """dU' per (position, image) over that image's rows and columns, gathered back to channel order and added in ascending image
    order, against a float64 reference computed on the CPU; the dense kernel on the same operands sets the scale. Same terms, another
    order (per-image chains of 1/n the length, then n - 1 additions): the bound is 2 x the dense form's rel-L2."""
    C, T = C0 + C1, n * Ti
    mask, drop, xt, xc, dyt, ks, pl = _operands(P, n, Ti, C0, C1, Kout, 13 * P + n + Kout)
    ref = torch.bmm(dyt.double().cpu().transpose(1, 2), xt.double().cpu())                 # [P][K][C]

    def args(x, batch, rows):
        a = MssConvArgs()
        a.x = ptr(x)
        a.N, a.H, a.W, a.C, a.ldx = 1, 1, rows, C, C
        a.OH, a.OW, a.K, a.Kpad = 1, rows, Kout, Kout
        a.R, a.S, a.stride, a.dil, a.pad = 1, 1, 1, 1, 0
        a.batch, a.x_bs, a.y_bs = batch, rows * C, rows * Kout
        return a
    a0 = args(xt, P, T)
    nbytes = _lib.value("mss_conv2d_wgrad_workspace_bytes", ctypes.byref(a0), C)
    ws = torch.empty(max(nbytes, 4) // 4, device="cuda")
    du0 = _with_canary(P * Kout * C)
    call("mss_conv2d_wgrad_f32", ctypes.byref(a0), ptr(dyt), Kout, ptr(du0), C, ptr(ws), nbytes)
    a1 = args(xc, P * n, Ti)
    a1.k_steps, a1.k_base, a1.k_imgs = ptr(drop.k_steps), C0 // 16, n
    assert _lib.value("mss_conv2d_wgrad_workspace_bytes", ctypes.byref(a1), C) == 0
    du1 = _with_canary(P * n * Kout * C)
    call("mss_conv2d_wgrad_f32", ctypes.byref(a1), ptr(dyt), Kout, ptr(du1), C, None, 0)
    assert torch.isnan(du0[P * Kout * C:]).all() and torch.isnan(du1[P * n * Kout * C:]).all()
    dun = du1[:P * n * Kout * C].view(P, n, Kout, C)
    for i in range(n):
        ext = C0 + 16 * ks[i]
        done = -(-ext // 128) * 128                           # whole 128-column tiles are written or left alone
        assert not torch.isnan(dun[:, i, :, :done]).any()
        assert float(dun[:, i, :, ext:done].abs().max() if done > ext else 0.0) == 0.0     # columns behind the extent inside a tile
        assert torch.isnan(dun[:, i, :, done:]).all()
    # the gather the projection pack does (mss_conv2d_pack_weights_f32 with `col`), here on [P] "taps" of 1 x 1: exact zeros for the
    # channels no image kept, the images added in ascending order
    got = torch.empty((P, Kout, C), device="cuda")
    src = dun.permute(1, 2, 3, 0).contiguous()               # [n][K][C][P]: P in the place of the R * S taps
    call("mss_conv2d_pack_weights_f32", ptr(src), ptr(got), Kout, C, P, 1, Kout, C, 0, ptr(drop.col), n, C0)
    nobody = (mask == 0).all(dim=0)
    assert bool(nobody.any()) and float(got[:, :, C0:][:, :, nobody].abs().max()) == 0.0
    e0, e1 = _rel_l2(du0[:P * Kout * C].view(P, Kout, C), ref), _rel_l2(got, ref)
    print(f"aspp dropped wgrad P={P} n={n} rows/img={Ti} C={C0}+{C1} K={Kout}: rel-L2 dense {e0:.3e} compact {e1:.3e} ratio {e1 / e0:.3f}")
    assert e1 <= 2.0 * e0, (e1, e0)


def _factored(n, H, W, C0, C1, per_sample=True, mask=True):
    a0, a1 = K.Act.zeros(n, H, W, C0, "cuda"), K.Act.zeros(n, H, W, C1, "cuda")
    aff0 = (torch.ones(C0, device="cuda"), torch.zeros(C0, device="cuda"))
    shape = (n, C1) if per_sample else (C1,)
    aff1 = (torch.ones(shape, device="cuda"), torch.zeros(shape, device="cuda"))
    return K.FactoredAct(a0, aff0, a1, aff1, torch.ones((n, C1), device="cuda") if mask else None)


def test_gate_leaves_other_shapes_and_the_split_route_dense(monkeypatch):
    w = [torch.zeros((256, 256, 3, 3), device="cuda")] * 3
    assert K.aspp_dropped_wanted(_factored(2, 8, 8, 128, 128), w)
    assert not K.aspp_dropped_wanted(_factored(2, 8, 8, 128, 128, mask=False), w)                  # eval: no Dropout2d
    assert not K.aspp_dropped_wanted(_factored(2, 8, 8, 128, 128, per_sample=False, mask=False), w)
    assert not K.aspp_dropped_wanted(_factored(2, 8, 8, 232, 24), w)                               # fewer than 48 channels behind the mask
    assert not K.aspp_dropped_wanted(_factored(2, 8, 8, 64, 96), [torch.zeros((256, 160, 3, 3), device="cuda")] * 3)   # C % 128
    assert not K.aspp_dropped_wanted(_factored(2, 8, 8, 128, 128), [torch.zeros((192, 256, 3, 3), device="cuda")] * 3)   # K % 128
    monkeypatch.setenv("MSS_ASPP_DROPOUT_COMPACT", "0")
    assert not K.aspp_dropped_wanted(_factored(2, 8, 8, 128, 128), w)
    monkeypatch.delenv("MSS_ASPP_DROPOUT_COMPACT")
    K.set_gemm_route("bf16x3")
    try:
        assert not K.aspp_dropped_wanted(_factored(2, 8, 8, 128, 128), w)
    finally:
        K.set_gemm_route(None)
    # a map outside the transform's gate (a tile edge of 2: the transform is not taken at all) plans the caller's dense path: no
    # dropped products, no X' and no average from the kernel; nothing raises
    plan = K.aspp_plan_for(_factored(2, 8, 8, 128, 128), (12, 24, 36), w)
    assert plan.tiles is None and not plan.dropped and not plan.single_read and not plan.gap_from_kernel and plan.materialise
    torch.cuda.synchronize()
