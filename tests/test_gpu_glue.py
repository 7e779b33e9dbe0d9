"""csrc/glue.hip and csrc/norm.hip kernel by kernel: exact on integer data, float64 on random data, one case on each side of
every branch and loop bound of the launch plans.

Reductions run on small non-zero integers stored as float32 (uniform in {-4..-1, 1..4}: every element, hence every row of
every channel quad, is non-zero), sized so that every partial sum stays below 2^24. Any order of summation then gives the
same exactly representable number and the comparison is `==`: one missing, doubled or misplaced row fails whatever its
position. The same entry points then run on random float data against float64 with the bounds of the existing tests.

Launch plans (read off the code; `splits` / `gy` are asserted through mss_colsum_workspace_floats and
mss_col_reduce_accum_doubles, the GroupNorm chunk count through mss_groupnorm_stat_offset, so a change of plan cannot turn
an edge case into an ordinary one unnoticed):

colsum_plan(N, HW, C) -- colsum / gap                        gx = ceil(C/64); splits = min(2048 // (gx*N), ceil(HW/128)) >= 1;
                                                             rps = ceil(HW/splits); splits = ceil(HW/rps)
  one split, one row                                         (1, 1, 4)
  one split, HW on the 128-row boundary                      (1, 128, 64), (3, 45, 64)
  two splits, short last split (65 + 64), ld > C             (2, 129, 20), (3, 129, 4)
  rps % 16 != 0 (the 16 row lanes end unevenly)              rps 65, 121, 125, 111, 100, 318 below
  C % 64 != 0 (lanes with c >= C idle)                       C = 4, 20, 48, 96, 124, 132, 304
  N*C % 16 != 0 (ragged last block of colsum_final_kernel)   (1, 1, 4), (3, 129, 4), (2, 129, 20), (3, 300, 20), (2, 640, 124)
  splits == 16 / 17 / 33 / 40 (one trip, one extra lane,     (1, 2048, 128) / (1, 2049, 128) / (1, 4097, 48) / (1, 5000, 96)
      two full trips + 1, ragged trips of the 16 split lanes)
  gx*N == 1024 -> cap 2; gx*N > 2048 -> 2048 // (gx*N) == 0  (16, 130, 4096) / (33, 130, 4096)
  capped by 2048 // (gx*N) on a long map                     (2, 32768, 4096) [ASPP input: 16 splits], (1, 162624, 256) [a Linear's
                                                             bias gradient: 512 splits of 318 rows, last 126]
  C = 1280, 304, 132                                         (2, 300, 1280), (1, 777, 304), (3, 1000, 132)

col_reduce_grid(M, C) + col_reduce2 -- bn_stats, bn_stats_partials, bn_relu_bwd_reduce
                                                             QPB = min(C/4, 32); gx = ceil(C/4 / QPB); RPB = 256 // QPB;
                                                             gy = min(2048 // gx, ceil(M/64)) >= 1; rpb = ceil(M/gy)
  C/4 < 32 / == 32 / > 32 (second block: one live quad)      C = 124 / 128 / 132
  C/4 does not divide 256 (idle lanes, ty >= RPB)            C = 20 (RPB 51), 48 (21), 96 (10), 124 (8, 248 threads)
  ragged last quad group                                     C = 304 (76 quads = 32 + 32 + 12), C = 1280 (10 groups)
  rows per thread 1 / 3|4 / 4 / 4|5 / 8 (four-row trips      M = 1, 8 / 31 / 32 / 33 / 64 at C = 128 (RPB 8, gy 1)
      against the tail loop)
  gy 1 -> 2                                                  M = 64 -> 65 at C = 128
  empty trailing row blocks (rpb * (gy - 1) >= M)            (13057, 1280) [gy 204, rpb 65: 3 empty], (131077, 128) [31 empty],
                                                             (162624, 256) [1 empty]
  more than 256 rows per thread: the flush to float64        (131584, 4096): gy 64, rpb 2056, 257 rows per thread: 2.16 GB, the
                                                             largest input of the module (3.3 GiB at its peak; the module's
                                                             highest peak, 4.5 GiB, is bn_relu_bwd_apply at 162624 x 256 with
                                                             its float64 reference)
  col_reduce_final_kernel, nparts <= 64 / 65 / 70 /          gy = 1..47 above / (4100, 256) / (4480, 128) /
      1024 / 1094 (> 1024: second trip) / 2048               (162624, 256) / (70000, 128) / (131077, 128)
  production                                                 (65536, 4096) [2 x 128 x 256 ASPP input: gy 64], (162624, 256)
bn_final_finalize_kernel (mss_bn_fold_train_from_partials_f32): the same row loop over nparts = gy of the partials' own grid
  gy 1 / 3 / 65 / 1024 / 2048                                nparts = 7 / 189 / 4100 (C 256) / 65536 (C 256) / 131077 (C 128)
gap_from_partials_kernel: 4 block lanes x 8 rows per trip    blocks per image 1, 3, 4, 5, 31, 32, 33, 65, 512; C = 4, 20, 64, 68, 4096
bn_relu_bwd_apply plan (not exported; mirrored by _apply_plan below)
                                                             QPB = min(C/4, 64); gx = ceil(C/4 / QPB); RPB = 256 // QPB;
                                                             gy = min(4096 // gx, ceil(M / (8*RPB))) >= 1 (the 65535 cap
                                                             cannot bind: 4096 // gx <= 4096)
  C/4 < 64 / == 64 / > 64                                    C = 252 / 256 / 260
  rows per thread 1 / 3|4 / 4 / 4|5 / 8; gy 1 -> 2           M = 1, 3, 4 / 13 / 16 / 17 / 32; 33 at C = 256 (RPB 4)
  QPB = 1 (RPB 256), QPB = 5 (RPB 51, idle lanes)            C = 4, C = 20
  gy capped at 4096 // gx                                    (162624, 256) [gy 4096], (9000, 4096) [gx 16, gy 256]
  ragged last quad group                                     C = 304

upsample_ac backward: the fast kernel when sw > 0 and 2/sw + 5 <= 14 and IH, N <= 65535, else the generic grid-stride one
  both sides of the switch                                   IW 10 -> OW 41 (13.9: fast) / 42 (14.1: generic); IW == 1 (sw = 0)
  both kernels on the same rows                              IH = OH = 65536 (generic; also wraps its 4096-block grid) against
                                                             the first 65535 rows through the fast kernel
GroupNorm chunk plan                                         chunks = min(ceil(HW/256), 512); rpc = ceil(HW/chunks);
                                                             chunks = ceil(HW/rpc)
  HW 1, 255, 256 / 257 / 1025 / 131072 / 131073 / 131372     1 chunk / 2 (129 + 128) / 5 x 205 / 512 x 256 (on the cap) /
                                                             511 (rpc 257, last 3) / 512 (rpc 257, last 45)
add_layernorm_bwd row blocks                                 blocks = min(ceil(rows/64), 1024); rpb = ceil(rows/blocks)
  rows 1, 3, 4, 5 / 1023 / 50001 / 70001                     1 block / 16 (last 63) / 782 (last 17) / 1015 of 69 (capped, last 35)

Out of scope, on purpose: NaN inputs of maxpool3s2 (the kernel uses fmaxf, which drops a NaN where torch propagates it;
neither behaviour is asserted), and BatchNorm / GroupNorm inputs whose mean is large against their spread (the one-pass
variance). ReLU-gated backward cases use data whose pre-activation stays away from zero (asserted on the float64
reference), so that the float32 and the float64 gate agree on every element; every output element is compared.

Bilinear references. `F.interpolate` on float64 input also computes the source index in float64; ATen's float32 kernels
(and these) compute it in float32, which moves a tap weight by up to 2^-23 * extent -- 3e-5 on a 256-wide map, more than
the bound the existing tests use. So every case is held to TWO references: (B) a float64 blend with the float32
source-index arithmetic of ATen, at the existing bounds unchanged; (A) F.interpolate / its autograd in float64, at the
existing bounds plus the derived index term (see _index_term).
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAN = float("nan")
U = 2.0 ** -24                      # unit roundoff of float32
MSS_ERR_BAD_ARG, MSS_ERR_UNSUPPORTED = 1001, 1002


@pytest.fixture(scope="module")
def L():
    from multishiftseg_amd import _lib
    _lib.load()
    return _lib


def gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def ints(g, *shape):
    """float32 integers uniform in {-4..-1, 1..4} (no zeros), generated on the device."""
    x = torch.randint(0, 8, shape, device="cuda", dtype=torch.float32, generator=g)
    x -= 4
    x += (x >= 0)
    return x


def randn(g, *shape, mean=0.0, std=1.0):
    x = torch.randn(shape, device="cuda", dtype=torch.float32, generator=g)
    if std != 1.0:
        x *= std
    if mean != 0.0:
        x += mean
    return x


def at(t, floats):
    return ctypes.c_void_p(t.data_ptr() + 4 * floats)


def window(x, ld, c0=0):
    """x [..., C] inside a NaN buffer [..., ld] at column c0 -> (buffer, pointer to its first element)."""
    C = x.shape[-1]
    if ld == C and c0 == 0:
        x = x.contiguous()
        return x, at(x, 0)
    assert c0 % 4 == 0 and c0 + C <= ld
    buf = torch.full(tuple(x.shape[:-1]) + (ld,), NAN, device="cuda", dtype=torch.float32)
    buf[..., c0:c0 + C] = x
    return buf, at(buf, c0)


def nan_out(*shape, ld=None, c0=0, dtype=torch.float32):
    """NaN buffer [..., ld]; returns (buffer, view of the window [..., c0:c0+C], pointer to the window)."""
    C = shape[-1]
    ld = ld or C
    buf = torch.full(tuple(shape[:-1]) + (ld,), NAN, device="cuda", dtype=dtype)
    return buf, buf[..., c0:c0 + C], at(buf, c0)


def outside_is_nan(buf, c0, C):
    return bool(torch.isnan(buf[..., :c0]).all()) and bool(torch.isnan(buf[..., c0 + C:]).all())


def sum64(x, chunk=8192):
    """Column sums of x [M, C] in float64 on the device, a slab of rows at a time (exact on integer data)."""
    acc = torch.zeros(x.shape[1], device=x.device, dtype=torch.float64)
    for i in range(0, x.shape[0], chunk):
        acc += x[i:i + chunk].double().sum(0)
    return acc


def host(t):
    return t.detach().cpu().numpy()


def eq(got, want, msg=""):
    """Every element equal (as numbers: -0 == 0; a NaN equals nothing). Compared on the device; the host copy is only made to
    word the failure."""
    got, want = got.detach(), want.detach()
    assert got.shape == want.shape, (got.shape, want.shape, msg)
    if got.dtype != want.dtype:
        got, want = got.double(), want.double()
    if not bool((got == want).all()):
        np.testing.assert_array_equal(host(got).astype(np.float64), host(want).astype(np.float64), err_msg=msg)
        raise AssertionError(msg)


def close(got, want, rtol, atol, msg=""):
    """|got - want| <= atol + rtol * |want| on every element; atol may be a tensor of the same shape."""
    got, want = got.detach().double(), want.detach().double()
    assert got.shape == want.shape, (got.shape, want.shape, msg)
    err = (got - want).abs()
    bound = rtol * want.abs() + atol
    bad = ~(err <= bound)                        # also catches NaN
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{msg}: {int(bad.sum())} of {bad.numel()} elements outside rtol {rtol} atol "
                             f"{atol if not torch.is_tensor(atol) else 'tensor'}; first at {i}: got {float(got[i])!r} want "
                             f"{float(want[i])!r}; max |err| {float(err.nan_to_num(float('inf')).max()):.3e}")
    return float(err.max()) if err.numel() else 0.0


def sum_atol(base, rows, adds=38):
    """Absolute bound of a float32 per-channel sum over `rows` zero-mean unit-variance terms. Each float32 addition on an
    element's path through the two-stage sums rounds by at most 2^-24 of the partial sum it produces, and partial sums of
    such terms stay below 4 * sqrt(rows), so the bound is adds * 2^-24 * 4 * sqrt(rows). LayerNorm backward: 16 additions in
    a wave's row walk, 3 across waves, at most 13 in a lane of the ordered column sum, 6 tree levels = 38, i.e. 9.1e-6 *
    sqrt(rows) -- 9.5e-5 at the 111 rows of the existing test, its 1e-4. GroupNorm backward: at most 65 in the row walk of a
    chunk plus the combine over its row lanes (257 rows over RPB lanes, then RPB - 1), 25 in a lane of the ordered column sum
    (3 * 512 chunks over 64 lanes), 6 tree levels = 96. `base` (the existing bound) holds wherever it is the larger."""
    return max(base, adds * U * 4 * float(np.sqrt(rows)))


# ================================================================================================ colsum / gap
# (N, HW, C, ld, splits)
COLSUM_CASES = [
    (1, 1, 4, 4, 1), (3, 45, 64, 64, 1), (1, 128, 64, 72, 1), (2, 129, 20, 32, 2), (3, 129, 4, 8, 2),
    (1, 2048, 128, 128, 16), (1, 2049, 128, 132, 17), (1, 4097, 48, 48, 33), (1, 5000, 96, 100, 40),
    (16, 130, 4096, 4096, 2), (33, 130, 4096, 4096, 1), (2, 300, 1280, 1284, 3), (1, 777, 304, 304, 7),
    (3, 1000, 132, 136, 8), (2, 640, 124, 128, 5), (3, 300, 20, 20, 3), (1, 4096, 256, 256, 32),
    (2, 32768, 4096, 4096, 16), (1, 162624, 256, 256, 512),
]


def _ulps(got, want64):
    """|got - want| in units of the float32 spacing at |want| (want in float64)."""
    w32 = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - want64) / np.spacing(np.maximum(np.abs(w32), np.float32(1e-30))).astype(np.float64)


@pytest.mark.parametrize("N,HW,C,ld,splits", COLSUM_CASES)
def test_colsum_gap(L, N, HW, C, ld, splits):
    g = gen(N * 1000003 + HW * 101 + C)
    nws = L.value("mss_colsum_workspace_floats", N, HW, C)
    assert nws == splits * N * C, f"plan changed: {nws // (N * C)} splits, the case was chosen for {splits}"
    for kind in ("int", "float"):
        x = ints(g, N, HW, C) if kind == "int" else randn(g, N, HW, C, mean=0.3, std=2.0)
        buf, p = window(x, ld)
        want = torch.stack([sum64(x[n]) for n in range(N)])
        outs = {}
        for name in ("mss_colsum_nhwc_f32", "mss_gap_nhwc_f32"):
            ws = torch.full((nws,), NAN, device="cuda")
            y = torch.full((N, C), NAN, device="cuda")
            L.call(name, p, ld, L.ptr(y), N, HW, C, L.ptr(ws))
            outs[name] = y
        del buf, x
        mean = host(want) / HW
        if kind == "int":
            eq(outs["mss_colsum_nhwc_f32"], want, "colsum on integers")
            got = host(outs["mss_gap_nhwc_f32"])
            if HW & (HW - 1) == 0:
                np.testing.assert_array_equal(got.astype(np.float64), mean, err_msg="gap, HW a power of two")
            else:       # exact sum * fl(1/HW): one rounding in the reciprocal, one in the product
                assert np.isfinite(got).all() and _ulps(got, mean).max() <= 2.0, _ulps(got, mean).max()
        else:
            close(outs["mss_colsum_nhwc_f32"], want, 1e-5, 1e-4, "colsum")
            close(outs["mss_gap_nhwc_f32"], want / HW, 1e-5, 1e-6, "gap")


def test_colsum_gap_refusals(L):
    x = torch.ones(2, 8, 8, device="cuda")
    y, ws = torch.full((2, 8), NAN, device="cuda"), torch.full((64,), NAN, device="cuda")
    for name in ("mss_colsum_nhwc_f32", "mss_gap_nhwc_f32"):
        assert L.status(name, L.ptr(x), 8, L.ptr(y), 2, 8, 6, L.ptr(ws)) == MSS_ERR_BAD_ARG       # C % 4
        assert L.status(name, L.ptr(x), 6, L.ptr(y), 2, 8, 4, L.ptr(ws)) == MSS_ERR_BAD_ARG       # ld % 4
        assert L.status(name, L.ptr(x), 8, L.ptr(y), 2, 0, 8, L.ptr(ws)) == MSS_ERR_BAD_ARG       # HW <= 0
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(ws).all()
    assert L.value("mss_colsum_workspace_floats", 0, 8, 8) == 0


# blocks per image x C x N
@pytest.mark.parametrize("bpi,C,N", [(1, 4, 1), (3, 20, 2), (4, 64, 3), (5, 68, 1), (31, 20, 2), (32, 64, 1), (33, 68, 3),
                                     (65, 4, 2), (512, 4096, 2), (7, 19, 2)])
def test_gap_from_partials(L, bpi, C, N):
    HW = 64 * bpi
    g = gen(bpi * 977 + C)
    x = ints(g, N, HW, C)
    blocks = x.view(N * bpi, 64, C)
    part = torch.stack([blocks.sum(1), (blocks * blocks).sum(1)], 1).contiguous()       # [N*bpi][2][C], exact in float32
    y = torch.full((N, C), NAN, device="cuda")
    L.call("mss_gap_from_partials_f32", L.ptr(part), N, HW, C, L.ptr(y))
    mean = host(x.double().sum(1)) / HW
    got = host(y)
    if bpi & (bpi - 1) == 0:
        np.testing.assert_array_equal(got.astype(np.float64), mean)
    else:
        assert np.isfinite(got).all() and _ulps(got, mean).max() <= 2.0, _ulps(got, mean).max()
    xr = randn(g, N, HW, C, mean=0.3, std=2.0).view(N * bpi, 64, C)
    partr = torch.stack([xr.sum(1), (xr * xr).sum(1)], 1).contiguous()
    L.call("mss_gap_from_partials_f32", L.ptr(partr), N, HW, C, L.ptr(y))
    close(y, partr[:, 0].double().view(N, bpi, C).sum(1) / HW, 1e-5, 1e-6, "gap from random partials")
    y.fill_(NAN)
    assert L.status("mss_gap_from_partials_f32", L.ptr(part), N, HW - 28, C, L.ptr(y)) == MSS_ERR_UNSUPPORTED      # HW % 64
    torch.cuda.synchronize()
    assert torch.isnan(y).all()


# ================================================================================================ BatchNorm reductions
# (M, C, ld, gy)
COLRED_CASES = [
    (1, 4, 4, 1), (1, 128, 128, 1), (8, 128, 128, 1), (31, 128, 132, 1), (32, 128, 128, 1), (33, 128, 128, 1),
    (64, 128, 128, 1), (65, 128, 128, 2), (189, 20, 24, 3), (1000, 48, 48, 16), (700, 96, 96, 11), (640, 124, 128, 10),
    (640, 132, 132, 10), (900, 304, 304, 15), (3000, 1280, 1280, 47), (13057, 1280, 1280, 204), (4100, 256, 260, 65),
    (4480, 128, 128, 70), (70000, 128, 128, 1094), (131077, 128, 128, 2048), (100000, 4, 8, 1563),
    (65536, 4096, 4096, 64), (162624, 256, 256, 1024), (131584, 4096, 4096, 64),
]


def _accum(L, M, C, gy):
    n = L.value("mss_col_reduce_accum_doubles", M, C)
    assert n == 2 * C * (1 + gy), f"plan changed: gy {n // (2 * C) - 1}, the case was chosen for {gy}"
    return torch.full((n,), NAN, device="cuda", dtype=torch.float64)


def _bn_finalize_ref(s, q, M, gamma, beta, eps, mom, rm, rv):
    """float64 of bn_finalize_train_kernel's formula from the column sums s, q (float64)."""
    mean = s / M
    var = (q / M - mean * mean).clamp_min(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    ga = gamma.double() if gamma is not None else torch.ones_like(mean)
    be = beta.double() if beta is not None else torch.zeros_like(mean)
    scale = ga * invstd
    unbiased = var * M / (M - 1) if M > 1 else var
    return dict(scale=scale, shift=be - mean * scale, mean=mean, invstd=invstd,
                rm=(1 - mom) * rm.double() + mom * mean, rv=(1 - mom) * rv.double() + mom * unbiased)


def _check_fold(out, ref, msg):
    # test_batchnorm_train_eval holds y = x*scale + shift to 1e-5 / 1e-5 and the running statistics to 1e-5 / 1e-6
    close(out["scale"], ref["scale"], 1e-5, 1e-5, msg + " scale")
    close(out["shift"], ref["shift"], 1e-5, 1e-5, msg + " shift")
    close(out["mean"], ref["mean"], 1e-5, 1e-6, msg + " save_mean")
    close(out["invstd"], ref["invstd"], 1e-5, 1e-6, msg + " save_invstd")
    close(out["rm"], ref["rm"], 1e-5, 1e-6, msg + " running_mean")
    close(out["rv"], ref["rv"], 1e-5, 1e-6, msg + " running_var")


def _fold_buffers(g, C):
    return dict(scale=torch.full((C,), NAN, device="cuda"), shift=torch.full((C,), NAN, device="cuda"),
                mean=torch.full((C,), NAN, device="cuda"), invstd=torch.full((C,), NAN, device="cuda"),
                rm=randn(g, C, std=0.2), rv=torch.rand(C, device="cuda", generator=g) + 0.5)


@pytest.mark.parametrize("M,C,ld,gy", COLRED_CASES)
def test_bn_stats_and_bwd_reduce_exact(L, M, C, ld, gy):
    g = gen(M * 31 + C)
    big = M * C > (1 << 28)                       # the flush case: one 2.16 GB map, dy shares its storage
    x = ints(g, M, C)
    xb, xp = window(x, ld)
    acc = _accum(L, M, C, gy)
    L.call("mss_bn_stats_nhwc_f32", xp, M, C, ld, L.ptr(acc))
    s = sum64(x)
    q = torch.zeros_like(s)
    for i in range(0, M, 8192):
        q += x[i:i + 8192].double().square().sum(0)
    eq(acc[:C], s, "bn_stats sums")
    eq(acc[C:2 * C], q, "bn_stats sums of squares")
    # backward reduce with an identity fold: a = sum dy * (x > 0), b = sum dy * (x > 0) * x (relu) / sum dy, sum dy * x (no relu)
    dy = x if big else ints(g, M, C)
    db, dp = (xb, xp) if big else window(dy, ld)
    one, zero = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    for relu in (1, 0):
        acc.fill_(NAN)
        L.call("mss_bn_relu_bwd_reduce_f32", dp, ld, xp, ld, M, C, L.ptr(one), L.ptr(zero), L.ptr(zero), L.ptr(one), relu, L.ptr(acc))
        a, b = torch.zeros_like(s), torch.zeros_like(s)
        for i in range(0, M, 8192):
            xs, ds = x[i:i + 8192].double(), dy[i:i + 8192].double()
            dz = ds * (xs > 0) if relu else ds
            a += dz.sum(0)
            b += (dz * xs).sum(0)
        eq(acc[:C], a, f"bwd reduce sum dz, relu {relu}")
        eq(acc[C:2 * C], b, f"bwd reduce sum dz * xhat, relu {relu}")
    if M * C > (1 << 26):                        # keeps the float64 reference of dx below 1 GB
        return
    # the parameter gradients ride on those sums: dbeta += sum dz, dgamma += sum dz * xhat, exactly (accum holds relu = 0)
    dg0, db0 = ints(g, C), ints(g, C)
    dg, dbt = dg0.clone(), db0.clone()
    dxb, dxv, dxp = nan_out(M, C, ld=ld)
    L.call("mss_bn_relu_bwd_apply_f32", dp, ld, xp, ld, dxp, ld, M, C, None, L.ptr(one), L.ptr(zero), L.ptr(zero), L.ptr(one), 0,
           L.ptr(acc), L.ptr(dg), L.ptr(dbt))
    eq(dg, dg0.double() + b, "dgamma")
    eq(dbt, db0.double() + a, "dbeta")
    assert outside_is_nan(dxb, 0, C)
    # dx = dz - mean(dz) - x * mean(dz * x) of the same identity fold against float64 (bound of test_bn_relu_backward)
    want = dy.double() - a / M - x.double() * (b / M)
    close(dxv, want, 1e-4, 1e-5, "dx")


@pytest.mark.parametrize("M,C,ld,gy", [c for c in COLRED_CASES if c[0] * c[1] <= (1 << 28)])
def test_bn_stats_finalize_random(L, M, C, ld, gy):
    g = gen(M * 37 + C + 1)
    x = randn(g, M, C, mean=0.4, std=1.5)                     # |mean| well inside sigma: the one-pass variance is out of scope
    xb, xp = window(x, ld)
    acc = _accum(L, M, C, gy)
    L.call("mss_bn_stats_nhwc_f32", xp, M, C, ld, L.ptr(acc))
    s = sum64(x)
    q = torch.zeros_like(s)
    for i in range(0, M, 8192):
        q += x[i:i + 8192].double().square().sum(0)
    close(acc[:C], s, 1e-5, 1e-4, "sums")                       # the bounds of colsum
    close(acc[C:2 * C], q, 1e-5, 1e-4, "sums of squares")
    gamma, beta = torch.rand(C, device="cuda", generator=g) + 0.5, randn(g, C, std=0.3)
    out = _fold_buffers(g, C)
    ref = _bn_finalize_ref(acc[:C].clone(), acc[C:2 * C].clone(), M, gamma, beta, 1e-5, 0.1, out["rm"], out["rv"])
    L.call("mss_bn_finalize_train_f32", L.ptr(acc), M, C, L.ptr(gamma), L.ptr(beta), 1e-5, 0.1, L.ptr(out["rm"]), L.ptr(out["rv"]),
           L.ptr(out["scale"]), L.ptr(out["shift"]), L.ptr(out["mean"]), L.ptr(out["invstd"]))
    _check_fold(out, ref, "finalize of the kernel's sums")


# (nparts, C, gy of the partials' grid)
PARTIAL_CASES = [(1, 4, 1), (7, 20, 1), (189, 48, 3), (640, 124, 10), (640, 132, 10), (900, 304, 15), (512, 4096, 8), (4100, 256, 65),
                 (2541, 256, 40), (65536, 256, 1024), (70000, 128, 1094), (131077, 128, 2048), (13057, 1280, 204)]


@pytest.mark.parametrize("nparts,C,gy", PARTIAL_CASES)
def test_bn_stats_partials_and_fold(L, nparts, C, gy):
    g = gen(nparts * 41 + C)
    part = torch.stack([ints(g, nparts, C), ints(g, nparts, C) + 72], 1).contiguous()       # [nparts][2][C]: sums | sums of squares
    s, q = sum64(part[:, 0]), sum64(part[:, 1])
    acc = _accum(L, nparts, C, gy)
    L.call("mss_bn_stats_partials_f32", L.ptr(part), nparts, C, L.ptr(acc))
    eq(acc[:C], s, "partials: sums")
    eq(acc[C:2 * C], q, "partials: sums of squares")
    M = 64 * nparts
    gamma, beta = torch.rand(C, device="cuda", generator=g) + 0.5, randn(g, C, std=0.3)
    two = _fold_buffers(g, C)
    one = {k: v.clone() for k, v in two.items()}
    ref = _bn_finalize_ref(s, q, M, gamma, beta, 1e-5, 0.1, two["rm"], two["rv"])
    L.call("mss_bn_finalize_train_f32", L.ptr(acc), M, C, L.ptr(gamma), L.ptr(beta), 1e-5, 0.1, L.ptr(two["rm"]), L.ptr(two["rv"]),
           L.ptr(two["scale"]), L.ptr(two["shift"]), L.ptr(two["mean"]), L.ptr(two["invstd"]))
    acc.fill_(NAN)
    L.call("mss_bn_fold_train_from_partials_f32", L.ptr(part), nparts, C, L.ptr(acc), M, L.ptr(gamma), L.ptr(beta), 1e-5, 0.1,
           L.ptr(one["rm"]), L.ptr(one["rv"]), L.ptr(one["scale"]), L.ptr(one["shift"]), L.ptr(one["mean"]), L.ptr(one["invstd"]))
    eq(acc[:C], s, "fold from partials: sums")
    eq(acc[C:2 * C], q, "fold from partials: sums of squares")
    _check_fold(one, ref, "fold from partials")
    for k in one:                                # documented as bit-identical to the two-call path
        eq(one[k], two[k], f"fold from partials vs stats_partials + finalize: {k}")
    # no affine, no running statistics, no saved statistics
    sc, sh = torch.full((C,), NAN, device="cuda"), torch.full((C,), NAN, device="cuda")
    L.call("mss_bn_fold_train_from_partials_f32", L.ptr(part), nparts, C, L.ptr(acc), M, None, None, 1e-5, 0.1, None, None,
           L.ptr(sc), L.ptr(sh), None, None)
    close(sc, ref["invstd"], 1e-5, 1e-5, "scale without gamma")
    close(sh, -ref["mean"] * ref["invstd"], 1e-5, 1e-5, "shift without beta")


@pytest.mark.parametrize("C", [1, 19, 256, 257, 4096])
def test_bn_fold_eval(L, C):
    g = gen(C)
    gamma, beta = torch.rand(C, device="cuda", generator=g) + 0.5, randn(g, C, std=0.3)
    rm, rv = randn(g, C), torch.rand(C, device="cuda", generator=g) + 0.1
    for ga, be in ((gamma, beta), (None, None)):
        sc, sh = torch.full((C,), NAN, device="cuda"), torch.full((C,), NAN, device="cuda")
        L.call("mss_bn_fold_eval_f32", L.ptr(ga), L.ptr(be), L.ptr(rm), L.ptr(rv), 1e-5, C, L.ptr(sc), L.ptr(sh))
        inv = 1.0 / torch.sqrt(rv.double() + 1e-5)
        s64 = inv * (ga.double() if ga is not None else 1.0)
        close(sc, s64, 1e-5, 1e-6, "eval scale")
        close(sh, (be.double() if be is not None else 0.0) - rm.double() * s64, 1e-5, 1e-6, "eval shift")


def _apply_plan(M, C):
    C4 = C // 4
    QPB = min(C4, 64)
    gx, RPB = -(-C4 // QPB), 256 // QPB
    return gx, max(1, min(4096 // gx, -(-M // (8 * RPB)))), QPB, RPB


def _gapped(g, M, C):
    """Rows in +/- pairs with |x| in [1, 2.5): per-channel mean ~ 0 and no x-hat near zero, so relu(x-hat * gamma + beta) has
    the same gate in float32 and float64 for |beta| small against gamma."""
    v = (torch.rand(-(-M // 2), C, device="cuda", generator=g) * 1.5 + 1.0) * (ints(g, -(-M // 2), C).sign())
    return torch.stack([v, -v], 1).reshape(-1, C)[:M].contiguous()


# (M, C, ldx, lddy, lddx, gy of the mirrored plan)
APPLY_CASES = [(1, 256, 256, 256, 256, 1), (3, 256, 256, 256, 256, 1), (4, 256, 256, 256, 256, 1), (13, 256, 260, 264, 268, 1),
               (16, 256, 256, 256, 256, 1), (17, 256, 256, 256, 256, 1), (32, 256, 256, 256, 256, 1), (33, 256, 256, 256, 256, 2),
               (500, 252, 252, 256, 252, 16), (500, 260, 260, 260, 264, 16), (700, 304, 304, 304, 304, 22), (5000, 4, 8, 4, 12, 3),
               (300, 20, 20, 24, 20, 1), (9000, 4096, 4096, 4096, 4096, 256), (162624, 256, 256, 256, 256, 4096)]


@pytest.mark.parametrize("M,C,ldx,lddy,lddx,gy", APPLY_CASES)
def test_bn_relu_bwd_apply(L, M, C, ldx, lddy, lddx, gy):
    assert _apply_plan(M, C)[1] == gy
    g = gen(M * 43 + C)
    x, dy = _gapped(g, M, C), randn(g, M, C)
    xb, xp = window(x, ldx)
    db, dp = window(dy, lddy)
    gamma = torch.rand(C, device="cuda", generator=g) + 0.5
    beta = (torch.rand(C, device="cuda", generator=g) * 0.015 + 0.005) * ints(g, C).sign()
    gyr = L.value("mss_col_reduce_accum_doubles", M, C) // (2 * C) - 1
    acc = _accum(L, M, C, gyr)
    L.call("mss_bn_stats_nhwc_f32", xp, M, C, ldx, L.ptr(acc))
    st = _fold_buffers(g, C)
    L.call("mss_bn_finalize_train_f32", L.ptr(acc), M, C, L.ptr(gamma), L.ptr(beta), 1e-5, 0.1, None, None, L.ptr(st["scale"]),
           L.ptr(st["shift"]), L.ptr(st["mean"]), L.ptr(st["invstd"]))
    x64, d64 = x.double(), dy.double()
    mean = x64.mean(0)
    invstd = 1.0 / torch.sqrt(x64.var(0, unbiased=False) + 1e-5) if M > 1 else torch.full_like(mean, 1e-5 ** -0.5)
    xhat = (x64 - mean) * invstd
    z = xhat * gamma.double() + beta.double()
    assert float(z.abs().min()) > 1e-3, "test data must keep the ReLU gate away from zero"
    for relu in (1, 0):
        dz = d64 * (z > 0) if relu else d64
        acc.fill_(NAN)
        L.call("mss_bn_relu_bwd_reduce_f32", dp, lddy, xp, ldx, M, C, L.ptr(st["scale"]), L.ptr(st["shift"]), L.ptr(st["mean"]),
               L.ptr(st["invstd"]), relu, L.ptr(acc))
        close(acc[:C], dz.sum(0), 1e-4, 1e-4, f"sum dz, relu {relu}")
        close(acc[C:2 * C], (dz * xhat).sum(0), 1e-4, 1e-4, f"sum dz * xhat, relu {relu}")
        dg0, db0 = randn(g, C), randn(g, C)
        dg, dbt = dg0.clone(), db0.clone()
        dxb, dxv, dxp = nan_out(M, C, ld=lddx)
        L.call("mss_bn_relu_bwd_apply_f32", dp, lddy, xp, ldx, dxp, lddx, M, C, None, L.ptr(st["scale"]), L.ptr(st["shift"]),
               L.ptr(st["mean"]), L.ptr(st["invstd"]), relu, L.ptr(acc), L.ptr(dg), L.ptr(dbt))
        t1, t2, t3 = dz, dz.mean(0).expand_as(dz), xhat * (dz * xhat).mean(0)
        want = gamma.double() * invstd * (t1 - t2 - t3)
        # bounds of test_bn_relu_backward, plus the rounding of the three float32 terms dx is assembled from: 3 * 2^-24 of
        # their absolute sum. Nothing at ordinary scales (5e-7); at M = 1 the variance is 0, scale = gamma / sqrt(eps) ~ 300
        # and dx = 300*dz - 300*dz - 0 is left with the rounding of a fused product (2.8e-5 observed, 1e-4 allowed)
        terms = (gamma.double() * invstd).abs() * (t1.abs() + t2.abs() + t3.abs())
        close(dxv, want, 1e-4, 1e-5 + 3 * U * terms, f"dx, relu {relu}")
        close(dg, dg0.double() + (dz * xhat).sum(0), 1e-4, 1e-4, f"dgamma, relu {relu}")
        close(dbt, db0.double() + dz.sum(0), 1e-4, 1e-4, f"dbeta, relu {relu}")
        assert outside_is_nan(dxb, 0, C)
        # eval-mode form (no accum): dx = scale * dz, one float32 product
        dxb, dxv, dxp = nan_out(M, C, ld=lddx)
        L.call("mss_bn_relu_bwd_apply_f32", dp, lddy, xp, ldx, dxp, lddx, M, C, None, L.ptr(st["scale"]), L.ptr(st["shift"]),
               None, None, relu, None, None, None)
        eq(dxv, st["scale"] * (dy * (z > 0) if relu else dy), f"dx without statistics, relu {relu}")


def test_bn_refusals(L):
    x = torch.ones(8, 8, device="cuda")
    acc = torch.full((64,), NAN, device="cuda", dtype=torch.float64)
    v = torch.ones(8, device="cuda")
    assert L.status("mss_bn_stats_nhwc_f32", L.ptr(x), 8, 6, 8, L.ptr(acc)) == MSS_ERR_BAD_ARG
    assert L.status("mss_bn_stats_nhwc_f32", L.ptr(x), 8, 4, 6, L.ptr(acc)) == MSS_ERR_BAD_ARG
    assert L.status("mss_bn_stats_partials_f32", L.ptr(x), 4, 6, L.ptr(acc)) == MSS_ERR_BAD_ARG
    assert L.status("mss_bn_relu_bwd_reduce_f32", L.ptr(x), 8, L.ptr(x), 8, 8, 6, L.ptr(v), L.ptr(v), L.ptr(v), L.ptr(v), 1,
                    L.ptr(acc)) == MSS_ERR_BAD_ARG
    assert L.status("mss_bn_finalize_train_f32", L.ptr(acc), 0, 8, None, None, 1e-5, 0.1, None, None, L.ptr(v), L.ptr(v), None,
                    None) == MSS_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert torch.isnan(acc).all()
    assert L.value("mss_col_reduce_accum_doubles", 0, 8) == 16


# ================================================================================================ max-pool
@pytest.mark.parametrize("C,ld", [(4, 4), (64, 64), (68, 72), (4, 12)])
def test_maxpool3s2(L, C, ld):
    g = gen(C + ld)
    for H in (1, 2, 3, 7, 8):
        for W in (1, 2, 3, 7, 8):
            for kind in ("mixed", "negative", "neginf"):
                x = randn(g, 2, H, W, C)
                if kind == "negative":
                    x = -x.abs() - 0.5                                   # a zero used as padding would win everywhere
                elif kind == "neginf":
                    x[torch.rand(x.shape, device="cuda", generator=g) < 0.4] = float("-inf")
                OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
                xb, xp = window(x, ld)
                yb, yv, yp = nan_out(2, OH, OW, C, ld=ld + 4, c0=4)
                L.call("mss_maxpool3s2_nhwc_f32", xp, ld, yp, ld + 4, 2, H, W, C, OH, OW)
                want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
                assert tuple(want.shape) == (2, OH, OW, C)
                np.testing.assert_array_equal(host(yv), host(want), err_msg=f"{H}x{W} {kind}")
                assert outside_is_nan(yb, 4, C)
    y = torch.full((2, 4, 4, C), NAN, device="cuda")
    x = torch.ones(2, 8, 8, C, device="cuda")
    assert L.status("mss_maxpool3s2_nhwc_f32", L.ptr(x), C, L.ptr(y), C, 2, 8, 8, C, 3, 4) == MSS_ERR_BAD_ARG      # wrong OH
    assert L.status("mss_maxpool3s2_nhwc_f32", L.ptr(x), C, L.ptr(y), C, 2, 8, 8, C - 2, 4, 4) == MSS_ERR_BAD_ARG  # C % 4
    assert L.status("mss_maxpool3s2_nhwc_f32", L.ptr(x), C + 2, L.ptr(y), C, 2, 8, 8, C, 4, 4) == MSS_ERR_BAD_ARG  # ld % 4
    torch.cuda.synchronize()
    assert torch.isnan(y).all()


def test_maxpool3s2_grid_wraps(L):
    """2 x 258 x 258 x 16 = 2.1 M channel quads: twice round the 4096-block grid."""
    x = randn(gen(5), 2, 515, 515, 64)
    y = torch.full((2, 258, 258, 64), NAN, device="cuda")
    L.call("mss_maxpool3s2_nhwc_f32", L.ptr(x), 64, L.ptr(y), 64, 2, 515, 515, 64, 258, 258)
    assert torch.equal(y, F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1))


# ================================================================================================ bilinear pairs
def _taps(inn, out, align):
    """ATen's float32 source-index arithmetic (area_pixel_compute_source_index): i0, i1, l0, l1 per output index."""
    o = np.arange(out, dtype=np.float32)
    if align:
        scale = np.float32(inn - 1) / np.float32(out - 1) if out > 1 else np.float32(0)
        src = (scale * o).astype(np.float32)
    else:
        scale = np.float32(inn) / np.float32(out)
        src = ((o + np.float32(0.5)) * scale).astype(np.float32) - np.float32(0.5)
        src = np.maximum(src, np.float32(0))
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < inn - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1) - l1).astype(np.float32)
    return i0, i1, l0, l1


def _matrix(inn, out, align):
    """[out, inn] float64 interpolation matrix with those float32 taps."""
    i0, i1, l0, l1 = _taps(inn, out, align)
    W = np.zeros((out, inn))
    np.add.at(W, (np.arange(out), i0), l0.astype(np.float64))
    np.add.at(W, (np.arange(out), i1), l1.astype(np.float64))
    return torch.from_numpy(W).cuda()


def _support(W):
    """0/1 matrix of the taps an output can reach under either index arithmetic: W's support widened by one cell."""
    A = (W != 0).double()
    A[:, 1:] += (W != 0).double()[:, :-1]
    A[:, :-1] += (W != 0).double()[:, 1:]
    return (A > 0).double()


def _sep(Wy, Wx, x):
    """y[n, o, p, c] = sum_ij Wy[o, i] Wx[p, j] x[n, i, j, c] in float64."""
    t = torch.einsum("oi,nijc->nojc", Wy, x.double())
    return torch.einsum("pj,nojc->nopc", Wx, t)


def _index_term(IH, IW):
    """Source indices computed in float32 (a rounded scale times an index, rounded again) and in float64 differ by at most
    2 * 2^-24 * extent; a tap weight is that index minus an integer, so each axis moves a weight by at most this much."""
    return 2 * U * IH, 2 * U * IW


def _interp64(x, size, align):
    return F.interpolate(x.double().permute(0, 3, 1, 2), size=size, mode="bilinear", align_corners=align).permute(0, 2, 3, 1)


def _check_pair(x, gyt, up, upT, IH, IW, OH, OW, align, fwd_bound, tag):
    """up: x [N,IH,IW,C] -> [N,OH,OW,C] and upT: its transpose, both through the kernels. Forward and transpose against both
    references, the adjoint identity on positive data, one-hot gradients."""
    Wy, Wx = _matrix(IH, OH, align), _matrix(IW, OW, align)
    dy_, dx_ = _index_term(IH, IW)
    y = up(x)
    want_b = _sep(Wy, Wx, x)
    close(y, want_b, *fwd_bound, f"{tag} forward vs float64 blend of float32 taps")
    xd = x.double()
    Dx = float((xd[:, :, 1:] - xd[:, :, :-1]).abs().max()) if IW > 1 else 0.0
    Dy = float((xd[:, 1:] - xd[:, :-1]).abs().max()) if IH > 1 else 0.0
    close(y, _interp64(x, (OH, OW), align), fwd_bound[0], fwd_bound[1] + dx_ * Dx + dy_ * Dy, f"{tag} forward vs F.interpolate float64")
    # transpose
    gx = upT(gyt)
    close(gx, _sep(Wy.T.contiguous(), Wx.T.contiguous(), gyt), 1e-4, 1e-5, f"{tag} transpose vs float64 blend of float32 taps")
    leaf = x.double().requires_grad_(True)
    F.interpolate(leaf.permute(0, 3, 1, 2), size=(OH, OW), mode="bilinear", align_corners=align).backward(gyt.double().permute(0, 3, 1, 2))
    reach = _sep(_support(Wy).T.contiguous(), _support(Wx).T.contiguous(), gyt.abs())      # sum of |g| over the outputs a cell can touch
    close(gx, leaf.grad, 1e-4, 1e-5 + (dx_ + dy_) * reach, f"{tag} transpose vs float64 autograd")
    # adjoint identity on positive data (no cancellation inside a blend, so each float32 output is within a few ulp of its
    # own magnitude and the two inner products may differ by 8 * 2^-24 of their absolute sums)
    xp_, gp_ = x.abs() + 0.5, gyt.abs() + 0.5
    yp, gxp = up(xp_), upT(gp_)
    lhs, rhs = (yp.double() * gp_.double()).sum(), (xp_.double() * gxp.double()).sum()
    bound = 8 * U * ((xp_.double() * gxp.double()).abs().sum() + (yp.double() * gp_.double()).abs().sum())
    assert abs(float(lhs - rhs)) <= float(bound), f"{tag} adjoint: <up x, g> {float(lhs)!r} vs <x, upT g> {float(rhs)!r}, bound {float(bound):.3e}"
    # one-hot gradients: the four corners, last column / last row mid-way, an interior pixel
    N, C = x.shape[0], x.shape[3]
    for (oy, ox) in sorted({(0, 0), (0, OW - 1), (OH - 1, 0), (OH - 1, OW - 1), (OH // 2, OW - 1), (OH - 1, OW // 2), (OH // 3, (2 * OW) // 3)}):
        hot = torch.zeros_like(gyt)
        hot[:, oy, ox, :] = 1.0
        got = upT(hot)
        want = (Wy[oy][:, None] * Wx[ox][None, :])[None, :, :, None].expand(N, IH, IW, C)
        np.testing.assert_array_equal(host(got) != 0, host(want) != 0, err_msg=f"{tag} one-hot at {(oy, ox)}: tap pattern")
        close(got, want, 1e-6, 1e-7, f"{tag} one-hot at {(oy, ox)}")          # a product of two float32 weights: 2 roundings
    return y, gx


# (N, C, ldx, ldy, IH, IW, OH, OW, fast transpose kernel?)
AC_CASES = [
    (2, 4, 4, 4, 11, 13, 22, 26, True), (1, 20, 24, 20, 11, 13, 41, 50, True), (2, 48, 48, 52, 7, 9, 7, 9, True),
    (1, 256, 256, 256, 4, 5, 32, 40, False), (1, 304, 304, 308, 5, 7, 20, 24, True), (2, 4, 8, 4, 1, 1, 5, 6, False),
    (1, 4, 4, 4, 1, 7, 1, 14, True), (1, 8, 8, 8, 5, 1, 10, 1, False), (1, 4, 4, 4, 3, 4, 1, 1, False), (1, 4, 4, 4, 6, 1, 3, 4, False),
    (2, 20, 20, 20, 22, 26, 11, 13, True), (1, 4, 4, 4, 41, 50, 7, 9, True), (1, 20, 20, 20, 9, 10, 30, 41, True),
    (1, 20, 20, 20, 9, 10, 30, 42, False), (1, 4, 4, 4, 3, 255, 5, 510, True), (1, 4, 4, 4, 3, 256, 5, 512, True),
    (1, 4, 4, 4, 3, 257, 5, 514, True), (1, 20, 20, 20, 2, 26, 3, 51, True), (1, 4, 4, 4, 3, 128, 4, 255, True),
    (1, 4, 4, 4, 3, 129, 4, 257, True), (1, 20, 20, 20, 128, 256, 1024, 2048, False),
]


def _ac_fast(IW, OW):
    sw = np.float32(IW - 1) / np.float32(OW - 1) if OW > 1 else np.float32(0)
    return bool(sw > 0 and np.float32(2) / sw + np.float32(5) <= np.float32(14))


@pytest.mark.parametrize("N,C,ldx,ldy,IH,IW,OH,OW,fast", AC_CASES)
def test_upsample_ac_pair(L, N, C, ldx, ldy, IH, IW, OH, OW, fast):
    assert _ac_fast(IW, OW) == fast, "the case no longer sits on the side of the kernel switch it was chosen for"
    g = gen(IH * 1009 + OW + C)

    def up(x):
        xb, xp = window(x, ldx)
        yb, yv, yp = nan_out(N, OH, OW, C, ld=ldy)
        L.call("mss_upsample_ac_nhwc_f32", xp, ldx, yp, ldy, N, IH, IW, OH, OW, C)
        assert outside_is_nan(yb, 0, C)
        return yv

    def upT(gy):
        gb, gp = window(gy, ldy)
        db, dv, dp = nan_out(N, IH, IW, C, ld=ldx)
        L.call("mss_upsample_ac_nhwc_bwd_f32", gp, ldy, dp, ldx, N, IH, IW, OH, OW, C)
        assert outside_is_nan(db, 0, C)
        return dv

    _check_pair(randn(g, N, IH, IW, C), randn(g, N, OH, OW, C), up, upT, IH, IW, OH, OW, True, (1e-5, 5e-6), "align-corners")


def test_upsample_ac_bwd_kernels_agree(L):
    """65536 rows (identity along y, so rows are independent) force the generic grid-stride kernel, and its 1.3 M quads wrap
    the 4096-block grid; the first 65535 rows through the fast kernel must give the same gradient."""
    IH, IW, OW, C = 65536, 20, 39, 4
    assert _ac_fast(IW, OW)
    gy = randn(gen(11), 1, IH, OW, C)
    slow = torch.full((1, IH, IW, C), NAN, device="cuda")
    L.call("mss_upsample_ac_nhwc_bwd_f32", L.ptr(gy), C, L.ptr(slow), C, 1, IH, IW, IH, OW, C)
    fast = torch.full((1, IH - 1, IW, C), NAN, device="cuda")
    L.call("mss_upsample_ac_nhwc_bwd_f32", L.ptr(gy), C, L.ptr(fast), C, 1, IH - 1, IW, IH - 1, OW, C)
    Wx = _matrix(IW, OW, True)
    want = torch.einsum("pj,nopc->nojc", Wx, gy.double())
    close(slow, want, 1e-4, 1e-5, "generic kernel")
    close(fast, want[:, :IH - 1], 1e-4, 1e-5, "fast kernel")
    close(fast, slow[:, :IH - 1], 1e-4, 1e-5, "fast vs generic kernel")


def test_upsample_refusals(L):
    x = torch.ones(1, 2, 2, 8, device="cuda")
    y = torch.full((1, 4, 4, 8), NAN, device="cuda")
    P = L.ptr
    assert L.status("mss_upsample_ac_nhwc_f32", P(x), 8, P(y), 8, 1, 2, 2, 65536, 4, 8) == MSS_ERR_UNSUPPORTED
    assert L.status("mss_upsample_ac_nhwc_f32", P(x), 8, P(y), 8, 1, 2, 2, 4, 4, 6) == MSS_ERR_BAD_ARG
    assert L.status("mss_upsample_ac_nhwc_f32", P(x), 6, P(y), 8, 1, 2, 2, 4, 4, 4) == MSS_ERR_BAD_ARG
    assert L.status("mss_upsample_ac_nhwc_f32", P(x), 8, P(y), 6, 1, 2, 2, 4, 4, 4) == MSS_ERR_BAD_ARG
    assert L.status("mss_upsample_ac_nhwc_bwd_f32", P(x), 8, P(y), 8, 1, 4, 4, 2, 2, 6) == MSS_ERR_BAD_ARG
    assert L.status("mss_upsample_ac_nhwc_bwd_f32", P(x), 6, P(y), 8, 1, 4, 4, 2, 2, 4) == MSS_ERR_BAD_ARG
    assert L.status("mss_upsample_bilinear_add_nhwc_f32", P(x), 8, 32, 1, 2, 2, P(y), 8, P(y), 8, 65536, 4, 8) == MSS_ERR_UNSUPPORTED
    assert L.status("mss_upsample_bilinear_add_nhwc_f32", P(x), 8, 32, 1, 2, 2, P(y), 8, P(y), 8, 4, 4, 6) == MSS_ERR_BAD_ARG
    assert L.status("mss_upsample_bilinear_add_nhwc_f32", P(x), 6, 32, 1, 2, 2, P(y), 8, P(y), 8, 4, 4, 4) == MSS_ERR_BAD_ARG
    assert L.status("mss_upsample_bilinear_bwd_nhwc_f32", P(x), 8, 1, 2, 2, P(y), 8, 128, 65536, 4, 8, 0) == MSS_ERR_UNSUPPORTED
    assert L.status("mss_upsample_bilinear_bwd_nhwc_f32", P(x), 8, 1, 2, 2, P(y), 8, 128, 4, 4, 6, 0) == MSS_ERR_BAD_ARG
    assert L.status("mss_upsample_bilinear_bwd_nhwc_f32", P(x), 8, 1, 2, 2, P(y), 6, 128, 4, 4, 4, 0) == MSS_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and bool((x == 1).all())


# (N, C, ldt, ldl, ldy, IH, IW, OH, OW)
HP_CASES = [
    (2, 4, 4, 4, 4, 5, 7, 10, 14), (1, 20, 24, 20, 28, 5, 7, 11, 13), (2, 48, 48, 48, 48, 5, 7, 5, 7), (1, 256, 256, 256, 256, 3, 5, 24, 40),
    (1, 304, 304, 308, 304, 6, 5, 24, 20), (2, 4, 4, 4, 4, 1, 1, 5, 6), (1, 4, 4, 4, 4, 1, 7, 1, 14), (1, 8, 8, 8, 8, 5, 1, 10, 1),
    (1, 4, 4, 4, 4, 3, 4, 1, 1), (2, 20, 20, 20, 20, 22, 26, 11, 13), (1, 4, 4, 4, 4, 41, 50, 7, 9), (1, 4, 4, 4, 4, 3, 255, 5, 510),
    (1, 4, 4, 4, 4, 3, 256, 5, 512), (1, 4, 4, 4, 4, 3, 257, 5, 514), (1, 4, 4, 4, 4, 3, 128, 4, 255), (1, 4, 4, 4, 4, 3, 129, 4, 257),
    (1, 256, 256, 256, 256, 128, 256, 256, 512),
]


@pytest.mark.parametrize("N,C,ldt,ldl,ldy,IH,IW,OH,OW", HP_CASES)
def test_upsample_bilinear_pair(L, N, C, ldt, ldl, ldy, IH, IW, OH, OW):
    g = gen(IH * 1013 + OW + C)
    lat = randn(g, N, OH, OW, C)
    pad_rows = 3                                           # the top map lives in a token buffer: rows before and after each sample
    tss = (IH * IW + 2 * pad_rows) * ldt

    def top_buffer(x, fill):
        buf = torch.full((N, IH * IW + 2 * pad_rows, ldt), fill, device="cuda")
        if x is not None:
            buf[:, pad_rows:pad_rows + IH * IW, :C] = x.reshape(N, IH * IW, C)
        return buf

    def up_add(x, lat_):
        tb = top_buffer(x, NAN)
        lb, lp = window(lat_, ldl)
        yb, yv, yp = nan_out(N, OH, OW, C, ld=ldy)
        L.call("mss_upsample_bilinear_add_nhwc_f32", at(tb, pad_rows * ldt), ldt, tss, N, IH, IW, lp, ldl, yp, ldy, OH, OW, C)
        assert outside_is_nan(yb, 0, C)
        return yv

    def upT(gy, base=None):
        gb, gp = window(gy, ldy)
        tb = top_buffer(base, NAN)
        L.call("mss_upsample_bilinear_bwd_nhwc_f32", gp, ldy, N, OH, OW, at(tb, pad_rows * ldt), ldt, tss, IH, IW, C, 0 if base is None else 1)
        assert torch.isnan(tb[:, :pad_rows]).all() and torch.isnan(tb[:, pad_rows + IH * IW:]).all() and outside_is_nan(tb, 0, C)
        return tb[:, pad_rows:pad_rows + IH * IW, :C].reshape(N, IH, IW, C)

    x, gy = randn(g, N, IH, IW, C), randn(g, N, OH, OW, C)
    zero_lat = torch.zeros_like(lat)
    # test_groupnorm_layernorm_upsample_ops_vs_oracle holds lat + up(top) to 1e-5 / 1e-5
    _, gx = _check_pair(x, gy, lambda t: up_add(t, zero_lat), upT, IH, IW, OH, OW, False, (1e-5, 1e-5), "half-pixel")
    close(up_add(x, lat), lat.double() + _sep(_matrix(IH, OH, False), _matrix(IW, OW, False), x), 1e-5, 1e-5, "lateral + up-sampled")
    base = randn(g, N, IH, IW, C)
    eq(upT(gy, base), base + gx, "accumulate = 1 against destination + the accumulate = 0 result")


# ================================================================================================ GroupNorm
def _paired(g, N, HW, C, signs_only):
    """Channels in (v, -v) pairs: every group of every pixel sums to zero exactly; |v| = 1, or in [1, 2.5) (no x-hat near 0)."""
    s = ints(g, N, HW, C // 2).sign()
    v = s if signs_only else s * (torch.rand(N, HW, C // 2, device="cuda", generator=g) * 1.5 + 1.0)
    return torch.stack([v, -v], -1).reshape(N, HW, C)


# (N, HW, C, groups, chunks, ld of x / gy / dx, token rows before the level or None)
GN_CASES = [
    (1, 1, 32, 8, 1, 32, None), (3, 1, 256, 32, 1, 256, 2), (1, 255, 128, 32, 1, 132, None), (3, 256, 192, 48, 1, 192, 3),
    (1, 257, 256, 32, 2, 256, None), (3, 257, 32, 1, 2, 36, 1), (1, 1025, 1024, 32, 5, 1024, None), (3, 1025, 192, 24, 5, 192, 5),
    (1, 131072, 256, 32, 512, 256, None), (1, 131073, 128, 16, 511, 128, 4), (3, 131073, 32, 8, 511, 32, None),
    (1, 131372, 192, 48, 512, 192, None), (1, 131372, 256, 32, 512, 256, 7),
]


def _gn_ref(x, groups, gamma, beta, eps, relu, gy):
    N, HW, C = x.shape
    leaf = x.double().permute(0, 2, 1).contiguous().requires_grad_(True)          # [N, C, HW]
    ga, be = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    pre = F.group_norm(leaf, groups, ga, be, eps)
    y = torch.relu(pre) if relu else pre
    y.backward(gy.double().permute(0, 2, 1))
    return y.detach().permute(0, 2, 1), pre.detach().permute(0, 2, 1), leaf.grad.permute(0, 2, 1), ga.grad, be.grad


@pytest.mark.parametrize("N,HW,C,groups,chunks,ld,tok", GN_CASES)
def test_groupnorm(L, N, HW, C, groups, chunks, ld, tok):
    assert L.value("mss_groupnorm_stat_offset", N, HW, C) == N * chunks * 2 * (C // 4), "chunk plan changed"
    g = gen(HW * 53 + C + N)
    gamma = torch.rand(C, device="cuda", generator=g) + 0.5
    beta_small = (torch.rand(C, device="cuda", generator=g) * 0.05 + 0.02) * ints(g, C).sign()
    beta_any = randn(g, C)
    nws = L.value("mss_groupnorm_workspace_floats", N, HW, C, groups)
    nbw = L.value("mss_groupnorm_bwd_workspace_floats", N, HW, C, groups)
    off = L.value("mss_groupnorm_stat_offset", N, HW, C)
    S = HW + (tok or 0) + 2                              # token buffer [N, S, C]: the level starts at row tok
    # (data, eps, relu, beta, exact?)
    runs = [("random", 1e-5, 0, beta_any, False), ("gapped", 1e-5, 1, beta_small, False), ("signs", 0.0, 0, beta_small, True),
            ("signs", 0.0, 1, beta_small, True)]
    for data, eps, relu, beta, exact in runs:
        if data == "random":
            x = randn(g, N, HW, C, mean=0.5, std=2.0)
        else:
            x = _paired(g, N, HW, C, data == "signs")
        gy = ints(g, N, HW, C) if exact else randn(g, N, HW, C)
        xss = (HW + 3) * ld                               # samples further apart than dense
        xb = torch.full((N, HW + 3, ld), NAN, device="cuda")
        xb[:, :HW, :C] = x
        gb = torch.full((N, HW + 3, ld), NAN, device="cuda")
        gb[:, :HW, :C] = gy
        ws = torch.full((nws,), NAN, device="cuda")
        if tok is None:
            yb = torch.full((N, HW, ld), NAN, device="cuda")
            yp, ldy, yss, yv = at(yb, 0), ld, HW * ld, yb[:, :, :C]
        else:
            yb = torch.full((N, S, C), NAN, device="cuda")
            yp, ldy, yss, yv = at(yb, tok * C), C, S * C, yb[:, tok:tok + HW]
        L.call("mss_groupnorm_nhwc_f32", at(xb, 0), ld, xss, N, HW, C, groups, L.ptr(gamma), L.ptr(beta), eps, relu, yp, ldy, yss, L.ptr(ws))
        want_y, pre, want_dx, want_dg, want_db = _gn_ref(x, groups, gamma, beta, eps, relu, gy)
        if relu:
            assert float(pre.abs().min()) > 1e-3, "test data must keep the ReLU gate away from zero"
        tag = f"{data} relu {relu}"
        close(yv, want_y, 1e-4, 1e-5, tag + " forward")
        if tok is None:
            assert outside_is_nan(yb, 0, C)
        else:
            assert torch.isnan(yb[:, :tok]).all() and torch.isnan(yb[:, tok + HW:]).all()
        if exact:       # mean 0 and variance 1 exactly, eps = 0: x-hat = +-1 and y = +-gamma + beta, one rounding
            y32 = torch.where(x > 0, gamma + beta, beta - gamma)
            eq(yv, torch.relu(y32) if relu else y32, tag + " forward on +-1 data")
        stat = ws[off:off + 2 * N * groups].clone()
        bws = torch.full((nbw,), NAN, device="cuda")
        dxb, dxv, dxp = nan_out(N, HW, C, ld=ld)
        dg, db = torch.full((C,), NAN, device="cuda"), torch.full((C,), NAN, device="cuda")
        L.call("mss_groupnorm_nhwc_bwd_f32", at(gb, 0), ld, xss, at(xb, 0), ld, xss, N, HW, C, groups, L.ptr(stat), L.ptr(gamma), L.ptr(beta),
               relu, dxp, ld, L.ptr(dg), L.ptr(db), L.ptr(bws))
        scale = max(1.0, float(want_dx.abs().max()))
        close(dxv, want_dx, 1e-3, 2e-5 * scale, tag + " dx")                 # bounds of test_groupnorm_upsample_backward_ops_vs_torch
        assert outside_is_nan(dxb, 0, C)
        if exact:       # x-hat = x = +-1: the sums are integers whatever the order (int64 here, not the autograd's float64 x-hat)
            gate = (y32 > 0) if relu else torch.ones_like(x, dtype=torch.bool)
            gi = (gy * gate).long()
            eq(dg, (gi * x.long()).sum((0, 1)), tag + " dgamma on integers")
            eq(db, gi.sum((0, 1)), tag + " dbeta on integers")
        else:
            close(dg, want_dg, 1e-3, sum_atol(1e-3, N * HW, 96), tag + " dgamma")
            close(db, want_db, 1e-3, sum_atol(1e-3, N * HW, 96), tag + " dbeta")
        del xb, gb, yb, dxb, want_y, pre, want_dx


def test_groupnorm_refusals(L):
    x = torch.ones(1, 4, 2048, device="cuda")
    y = torch.full((1, 4, 2048), NAN, device="cuda")
    v = torch.ones(2048, device="cuda")
    ws = torch.full((8192,), NAN, device="cuda")
    P = L.ptr
    for (C, groups, ld) in [(1028, 1, 1028), (32, 16, 32), (32, 3, 32), (30, 1, 32), (32, 8, 30)]:      # C/4 > 256, C/groups % 4, C % groups, C % 4, ld % 4
        assert L.status("mss_groupnorm_nhwc_f32", P(x), ld, 4 * ld, 1, 4, C, groups, P(v), P(v), 1e-5, 0, P(y), ld, 4 * ld, P(ws)) == MSS_ERR_UNSUPPORTED
        assert L.status("mss_groupnorm_nhwc_bwd_f32", P(x), ld, 4 * ld, P(x), ld, 4 * ld, 1, 4, C, groups, P(v), P(v), P(v), 0, P(y), ld, P(y), P(y),
                        P(ws)) == MSS_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(ws).all()


# ================================================================================================ add + LayerNorm
def _ln_ref(x, res, gamma, beta, eps, gy):
    a = x.double().requires_grad_(True)
    ga, be = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z = a + res.double() if res is not None else a
    y = F.layer_norm(z, (x.shape[1],), ga, be, eps)
    y.backward(gy.double())
    return y.detach(), a.grad, ga.grad, be.grad


@pytest.mark.parametrize("C", [256, 512, 768, 1024])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 1023, 50001])
def test_add_layernorm(L, C, rows):
    _layernorm_case(L, C, rows)


def test_add_layernorm_block_cap(L):
    """70 001 rows: the backward's row blocks are capped at 1024 (1015 blocks of 69 rows, the last with 35)."""
    assert L.value("mss_add_layernorm_bwd_workspace_floats", 70001, 256) == 1024 * 2 * 256
    _layernorm_case(L, 256, 70001)


def _layernorm_case(L, C, rows):
    g = gen(rows * 59 + C)
    gamma, beta = torch.rand(C, device="cuda", generator=g) + 0.5, randn(g, C)
    x, res, gy, gy2 = randn(g, rows, C), randn(g, rows, C, mean=0.2), randn(g, rows, C), randn(g, rows, C)
    nws = L.value("mss_add_layernorm_bwd_workspace_floats", rows, C)
    assert nws == min(-(-rows // 64), 1024) * 2 * C
    for r in (res, None):
        _layernorm_random(L, g, rows, C, nws, x, r, gy, gy2, gamma, beta)
    del x, res, gy, gy2
    _layernorm_exact(L, g, rows, C, nws, gamma)


def _layernorm_random(L, g, rows, C, nws, x, r, gy, gy2, gamma, beta):
    P = L.ptr
    tag = f"res {'yes' if r is not None else 'NULL'}"
    y, stat = torch.full((rows, C), NAN, device="cuda"), torch.full((rows, 2), NAN, device="cuda")
    L.call("mss_add_layernorm_f32", P(x), P(r), rows, C, P(gamma), P(beta), 1e-5, P(y), P(stat))
    want_y, want_dz, want_dg, want_db = _ln_ref(x, r, gamma, beta, 1e-5, gy)
    close(y, want_y, 1e-4, 1e-5, tag + " forward")          # bounds of test_groupnorm_layernorm_upsample_ops_vs_oracle
    z = x.double() + (r.double() if r is not None else 0)
    close(stat[:, 0], z.mean(1), 1e-5, 1e-6, tag + " saved mean")
    close(stat[:, 1], 1 / torch.sqrt(z.var(1, unbiased=False) + 1e-5), 1e-5, 1e-6, tag + " saved rstd")
    # the query variant: same y and statistics bit for bit, q = y + pos[row % pos_rows]
    for pos_rows in sorted({1, rows, max(1, rows // 3), min(rows, 7), rows + 2}):
        pos = randn(g, pos_rows, C)
        y2, stat2, q = torch.full((rows, C), NAN, device="cuda"), torch.full((rows, 2), NAN, device="cuda"), torch.full((rows, C), NAN, device="cuda")
        L.call("mss_add_layernorm_q_f32", P(x), P(r), rows, C, P(gamma), P(beta), 1e-5, P(y2), P(stat2), P(pos), pos_rows, P(q))
        eq(y2, y, tag + f" q variant y, pos_rows {pos_rows}")
        eq(stat2, stat, tag + " q variant statistics")
        eq(q, y + pos[torch.arange(rows, device="cuda") % pos_rows], tag + f" q, pos_rows {pos_rows}")
        del y2, stat2, q, pos
    del want_y, z
    # backward
    ws = torch.full((nws,), NAN, device="cuda")
    dz, dg, db = torch.full((rows, C), NAN, device="cuda"), torch.full((C,), NAN, device="cuda"), torch.full((C,), NAN, device="cuda")
    L.call("mss_add_layernorm_bwd_f32", P(gy), P(x), P(r), P(stat), rows, C, P(gamma), P(dz), P(dg), P(db), P(ws))
    close(dz, want_dz, 1e-3, 1e-5, tag + " dz")
    close(dg, want_dg, 1e-4, sum_atol(1e-4, rows), tag + " dgamma")
    close(db, want_db, 1e-4, sum_atol(1e-4, rows), tag + " dbeta")
    # two consumers: gradient gy + gy2 summed on load, plus the column sums of dz
    for second in (gy2, None):
        ws3 = torch.full((nws // 2 * 3,), NAN, device="cuda")
        dz2, dg2, db2, dzs = (torch.full((rows, C), NAN, device="cuda"), torch.full((C,), NAN, device="cuda"),
                              torch.full((C,), NAN, device="cuda"), torch.full((C,), NAN, device="cuda"))
        L.call("mss_add_layernorm_bwd_sum2_f32", P(gy), P(second), P(x), P(r), P(stat), rows, C, P(gamma), P(dz2), P(dg2), P(db2), P(dzs), P(ws3))
        if second is None:
            close(dz2, want_dz, 1e-3, 1e-5, tag + " sum2 without a second gradient: dz")
            close(dg2, want_dg, 1e-4, sum_atol(1e-4, rows), tag + " sum2 without a second gradient: dgamma")
            close(db2, want_db, 1e-4, sum_atol(1e-4, rows), tag + " sum2 without a second gradient: dbeta")
            close(dzs, want_dz.sum(0), 1e-4, sum_atol(1e-4, rows), tag + " column sums of dz")
        else:
            _, w_dz, w_dg, w_db = _ln_ref(x, r, gamma, beta, 1e-5, gy.double() + gy2.double())
            close(dz2, w_dz, 1e-3, 1e-5 * 1.5, tag + " sum2 dz")          # the summed gradient is sqrt(2) larger: atol scaled with it
            close(dg2, w_dg, 1e-4, sum_atol(1e-4, 2 * rows), tag + " sum2 dgamma")
            close(db2, w_db, 1e-4, sum_atol(1e-4, 2 * rows), tag + " sum2 dbeta")
            close(dzs, w_dz.sum(0), 1e-4, sum_atol(1e-4, 2 * rows), tag + " sum2 column sums of dz")


def _layernorm_exact(L, g, rows, C, nws, gamma):
    """Exact parameter gradients: integer x and gy with the statistics GIVEN as mean 0, rstd 1, so x-hat = x."""
    P = L.ptr
    xi, gi, g2i = ints(g, rows, C), ints(g, rows, C), ints(g, rows, C)
    stat1 = torch.tensor([0.0, 1.0], device="cuda").repeat(rows, 1).contiguous()
    ws3 = torch.full((nws // 2 * 3,), NAN, device="cuda")
    dz, dg, db, dzs = (torch.full((rows, C), NAN, device="cuda"), torch.full((C,), NAN, device="cuda"), torch.full((C,), NAN, device="cuda"),
                       torch.full((C,), NAN, device="cuda"))
    L.call("mss_add_layernorm_bwd_sum2_f32", P(gi), P(g2i), P(xi), None, P(stat1), rows, C, P(gamma), P(dz), P(dg), P(db), P(dzs), P(ws3))
    gs = gi.double() + g2i.double()
    eq(dg, (gs * xi.double()).sum(0), "dgamma on integers")
    eq(db, gs.sum(0), "dbeta on integers")
    gg = gs * gamma.double()
    close(dz, gg - gg.mean(1, keepdim=True) - xi.double() * (gg * xi.double()).mean(1, keepdim=True), 1e-3, 1e-4, "dz of the integer case")
    ws = torch.full((nws,), NAN, device="cuda")
    L.call("mss_add_layernorm_bwd_f32", P(gi), P(xi), None, P(stat1), rows, C, P(gamma), P(dz), P(dg), P(db), P(ws))
    eq(dg, (gi.double() * xi.double()).sum(0), "dgamma on integers, plain backward")
    eq(db, gi.double().sum(0), "dbeta on integers, plain backward")


def test_add_layernorm_refusals(L):
    P = L.ptr
    for C in (1280, 128):
        x = torch.ones(4, C, device="cuda")
        y, st, v = torch.full((4, C), NAN, device="cuda"), torch.full((4, 2), NAN, device="cuda"), torch.ones(C, device="cuda")
        ws = torch.full((3 * C,), NAN, device="cuda")
        assert L.status("mss_add_layernorm_f32", P(x), None, 4, C, P(v), P(v), 1e-5, P(y), P(st)) == MSS_ERR_UNSUPPORTED
        assert L.status("mss_add_layernorm_q_f32", P(x), None, 4, C, P(v), P(v), 1e-5, P(y), P(st), P(x), 4, P(y)) == MSS_ERR_UNSUPPORTED
        assert L.status("mss_add_layernorm_bwd_f32", P(x), P(x), None, P(x), 4, C, P(v), P(y), P(y), P(y), P(ws)) == MSS_ERR_UNSUPPORTED
        assert L.status("mss_add_layernorm_bwd_sum2_f32", P(x), None, P(x), None, P(x), 4, C, P(v), P(y), P(y), P(y), P(y), P(ws)) == MSS_ERR_UNSUPPORTED
        torch.cuda.synchronize()
        assert torch.isnan(y).all() and torch.isnan(st).all() and torch.isnan(ws).all()
    assert L.value("mss_add_layernorm_bwd_workspace_floats", 0, 256) == 0


# ================================================================================================ layout, pointwise
@pytest.mark.parametrize("N,HW,C", [(1, 1, 1), (2, 63, 65), (3, 64, 64), (1, 65, 63), (2, 130, 200), (1, 4096, 19), (2, 777, 256)])
def test_layout_conversions(L, N, HW, C):
    g = gen(HW * 61 + C)
    P = L.ptr
    ld, rows = C + 3, HW + 5                               # a pitch and a sample stride larger than dense
    x = randn(g, N, HW, C)
    xb = torch.full((N, rows, ld), NAN, device="cuda")
    xb[:, 2:2 + HW, :C] = x
    y = torch.full((N, C, HW), NAN, device="cuda")
    L.call("mss_nhwc_to_nchw_f32", at(xb, 2 * ld), ld, rows * ld, N, HW, C, P(y))
    eq(y, x.permute(0, 2, 1), "nhwc_to_nchw")
    gr = randn(g, N, C, HW)
    base = randn(g, N, rows, ld)
    for acc in (0, 1):
        dst = base.clone()
        L.call("mss_nchw_to_nhwc_strided_f32", P(gr), N, C, HW, at(dst, 2 * ld), ld, rows * ld, acc)
        want = base.clone()
        want[:, 2:2 + HW, :C] = gr.permute(0, 2, 1) + (base[:, 2:2 + HW, :C] if acc else 0)
        eq(dst, want, f"nchw_to_nhwc_strided accumulate {acc} (and nothing outside the level)")
    assert L.status("mss_nhwc_to_nchw_f32", P(xb), ld, rows * ld, N, 0, C, P(y)) == MSS_ERR_BAD_ARG
    assert L.status("mss_nchw_to_nhwc_strided_f32", P(gr), N, 0, HW, P(base), ld, rows * ld, 0) == MSS_ERR_BAD_ARG


@pytest.mark.parametrize("N,C,H,W,Cp", [(2, 3, 5, 7, 16), (1, 3, 4, 8, 4), (2, 19, 5, 8, 20), (2, 19, 5, 7, 32), (1, 64, 9, 9, 64),
                                        (3, 65, 8, 8, 128), (1, 200, 13, 20, 208)])
def test_nchw_to_nhwc_pad(L, N, C, H, W, Cp):
    """The per-pixel kernel (C < 16), the tiled one with 16-byte loads (HW % 4 == 0) and with scalar loads; pad channels zero."""
    x = randn(gen(C * 67 + W), N, C, H, W)
    y = torch.full((N, H, W, Cp), NAN, device="cuda")
    L.call("mss_nchw_to_nhwc_pad_f32", L.ptr(x), L.ptr(y), N, C, H, W, Cp)
    want = torch.zeros(N, H, W, Cp, device="cuda")
    want[..., :C] = x.permute(0, 2, 3, 1)
    eq(y, want)
    assert L.status("mss_nchw_to_nhwc_pad_f32", L.ptr(x), L.ptr(y), N, C, H, W, Cp + 2) == MSS_ERR_BAD_ARG


# (M or N*HW as (N, HW), C, ld)
@pytest.mark.parametrize("N,HW,C,ld", [(1, 1, 4, 4), (2, 63, 60, 64), (3, 64, 64, 64), (1, 65, 68, 72), (2, 300, 304, 304), (2, 600000, 4, 8),
                                       (1, 70000, 64, 64)])
def test_affine_relu_broadcast_rows(L, N, HW, C, ld):
    """Bit-equal to the torch expression on data whose products and sums are exact in float32 (integers times halves), so that
    a fused and an unfused multiply-add agree; then random data against float64 within the two roundings of x*scale + shift.
    (2, 600000, 4) and (1, 70000, 64) have more than 1 048 576 channel quads: the 4096-block grid-stride loops wrap."""
    g = gen(HW * 71 + C)
    P = L.ptr
    M = N * HW
    for kind in ("exact", "random"):
        if kind == "exact":
            x, v = ints(g, M, C), ints(g, N, C)
            scale, shift = ints(g, C) * 0.5, ints(g, C) * 0.25
        else:
            x, v = randn(g, M, C), randn(g, N, C)
            scale, shift = randn(g, C), randn(g, C)
        xb, xp = window(x, ld)
        for sc, sh in ((scale, shift), (None, None)):
            for relu in (0, 1):
                def ref(t):
                    t = t.double()
                    if sc is not None:
                        t = t * sc.double() + sh.double()
                    return torch.relu(t) if relu else t

                def check(got, src, tag):
                    if kind == "exact" or sc is None:
                        eq(got, ref(src), tag)
                    else:
                        mag = (src.double() * sc.double()).abs() + sh.double().abs()
                        close(got, ref(src), 0.0, 2 * U * mag, tag)
                yb, yv, yp = nan_out(M, C, ld=ld + 4, c0=4)
                L.call("mss_affine_relu_nhwc_f32", xp, ld, yp, ld + 4, M, C, P(sc), P(sh), relu)
                check(yv, x, f"affine_relu {kind} scale {sc is not None} relu {relu}")
                assert outside_is_nan(yb, 4, C)
                yb, yv, yp = nan_out(N, HW, C, ld=ld + 4, c0=4)
                L.call("mss_broadcast_rows_nhwc_f32", P(v), yp, ld + 4, N, HW, C, P(sc), P(sh), relu)
                check(yv, v[:, None, :].expand(N, HW, C), f"broadcast_rows {kind} scale {sc is not None} relu {relu}")
                assert outside_is_nan(yb, 4, C)
    y = torch.full((4, 8), NAN, device="cuda")
    x = torch.ones(4, 8, device="cuda")
    assert L.status("mss_affine_relu_nhwc_f32", P(x), 8, P(y), 8, 4, 6, None, None, 0) == MSS_ERR_BAD_ARG
    assert L.status("mss_affine_relu_nhwc_f32", P(x), 6, P(y), 8, 4, 4, None, None, 0) == MSS_ERR_BAD_ARG
    assert L.status("mss_broadcast_rows_nhwc_f32", P(x), P(y), 8, 1, 4, 6, None, None, 0) == MSS_ERR_BAD_ARG
    assert L.status("mss_broadcast_rows_nhwc_f32", P(x), P(y), 6, 1, 4, 4, None, None, 0) == MSS_ERR_BAD_ARG
    torch.cuda.synchronize()
    assert torch.isnan(y).all()
