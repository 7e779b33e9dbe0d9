"""The one case table of the exact weight-gradient tests: tests/test_wgrad_exact_cpu.py (reference, exactness condition, expected
plans, sensitivity; no GPU) and tests/test_gpu_wgrad_exact.py (every case through mss_conv2d_wgrad_f32, equality with float64).

All data are small integers, so every product and every partial sum is an integer or a half below 2^24 and an fp32 evaluation is
EXACT in any summation order: operands in [-2, 2], prologue scale in {0.5, 1, 2}, shift an integer in [-2, 2] (mul + add and a fused
fma give the same value). For the split-bf16 kernel such values are one bf16 term and two zero terms, so its six products are exact
as well.

A row's `expect` is the plan derived by hand from csrc/wgrad_route.h: kernel, splits, reduce group, plus full / wide_K / the two
parts where they matter. test_wgrad_exact_cpu.py compares it with what mss_conv2d_wgrad_plan answers, so a wrong derivation fails
there instead of quietly testing another kernel. The derivations, for the rules that recur:
  conv_wgrad_kernel: base = ktiles * ctiles * taps jobs; splits = split_search(base, 768, ceil(M / 128)), which for base * splits
    below 730 is the cap itself; rows per split = ceil(ceil(M / splits) / 16) * 16 and splits = ceil(M / rows per split).
  reduce group (wg_reduce_group): G doubles from 1 while G < 32, slab4 * G < 65536 and splits >= 8 G, slab4 = taps * Kpad * Cp / 4.
    The 1x1 / C = 64 / K = 19 rows have slab4 = 320: G = 2 for 8..15 splits, 4 for 16..31, 8 for 32..63, 16 for 64..127, 32 from 128.
"""
from dataclasses import dataclass, field

import torch

from ref_wgrad import out_size

KERNELS = ("conv32", "conv64", "conv128", "narrow", "tn_lds", "tn_wide", "tn_direct", "tn_direct_tail", "tn_direct_perimg", "tn_bf16x3",
           "two_part")          # include/mss_hip.h MSS_WG_*, in order


@dataclass
class Case:
    name: str
    intent: str
    expect: dict                    # kernel, splits, reduce_group [, full, wide_K, parts: [(kernel, splits, reduce_group)] * 2]
    seed: int
    # a convolution (batch == 0): x [N][H][W][C], R x R taps
    N: int = 1
    H: int = 1
    W: int = 1
    C: int = 32
    K: int = 19
    R: int = 1
    stride: int = 1
    dil: int = 1
    pad: int = 0
    # batch > 0: that many independent [T][K]^T [T][C] products (x [batch][T][C], dy [batch][T][K]); N = H = 1, W = T
    batch: int = 0
    T: int = 0
    ldx: int = 0                    # pixel stride of x (0: C) and the first channel of the slice
    x_c0: int = 0
    lddy: int = 0                   # the same for dy
    dy_c0: int = 0
    Kpad: int = 0                   # 0: K rounded up to 4
    Cp: int = 0                     # 0: C
    affine: str = ""                # "", "shared", "per_sample"
    relu: bool = False
    route: int = 0                  # MssConvArgs.route (1: the split-bf16 kernel where eligible)
    k_base: int = 0                 # per-image form: batch = positions * len(k_steps) entries ordered (position, image)
    k_steps: tuple = ()
    env: dict = field(default_factory=dict)     # MSS_WGRAD_* forcing switches
    ref: str = "cpu"                # "cpu": ref_wgrad.wgrad; "device": a float64 matmul on the device (1x1 / batched)

    def __post_init__(self):
        if self.batch:
            self.N, self.H, self.W = 1, 1, self.T
        self.ldx = self.ldx or self.C
        self.lddy = self.lddy or (self.K + 3) // 4 * 4        # (a pixel stride is a multiple of 4 floats)
        self.Kpad = self.Kpad or (self.K + 3) // 4 * 4
        self.Cp = self.Cp or self.C
        self.OH = out_size(self.H, self.R, self.stride, self.dil, self.pad)
        self.OW = out_size(self.W, self.R, self.stride, self.dil, self.pad)
        self.M = self.N * self.OH * self.OW

    @property
    def geometry(self):
        """The convolution-loader cases: what the reference and sensitivity checks of the CPU test run on."""
        return self.batch == 0 and self.ref == "cpu"

    @property
    def wrapper(self):
        """kernels.conv2d_wgrad can express the case: one position, its own padding of dwp, the native route."""
        return self.batch == 0 and self.Kpad == (self.K + 3) // 4 * 4 and self.Cp == self.C and self.route == 0


def operands(c):
    """The case's data on the CPU (float32, integer-valued): x [N][H][W][C] or [batch][T][C], dy [N][OH][OW][K] or [batch][T][K],
    scale / shift ([C], [N][C] or None)."""
    g = torch.Generator().manual_seed(c.seed)

    def ints(*shape):
        return torch.randint(-2, 3, shape, generator=g).float()
    if c.batch:
        x, dy = ints(c.batch, c.T, c.C), ints(c.batch, c.T, c.K)
    else:
        x, dy = ints(c.N, c.H, c.W, c.C), ints(c.N, c.OH, c.OW, c.K)
    scale = shift = None
    if c.affine:
        shape = (c.N, c.C) if c.affine == "per_sample" else (c.C,)
        scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, shape, generator=g)]
        shift = ints(*shape)
    return x, dy, scale, shift


def _conv(name, intent, expect, seed, **kw):
    return Case(name, intent, dict(zip(("kernel", "splits", "reduce_group"), expect)), seed, **kw)


FIRST = dict(N=2, H=14, W=13, C=32, R=3, pad=1, lddy=48, dy_c0=20)      # M = 364: 3 splits of 128, boundaries mid-row, image boundary at 182

CASES = [
    # ---- C1: conv_wgrad_kernel geometry ---------------------------------------------------------------------------------------
    # 9 jobs per split, cap ceil(364 / 128) = 3 -> 3 splits of 128 rows; fewer than 8 splits: the sequential reducer
    _conv("c3x3_k19", "3x3 / s1 / pad 1 over a dy slice, K % 4 == 3 (scalar dy loads), 3 splits mid-row and across the image boundary",
          ("conv32", 3, 1), 101, K=19, **FIRST),
    _conv("c3x3_k18", "the same, K % 4 == 2", ("conv32", 3, 1), 102, K=18, **FIRST),
    _conv("c3x3_k17", "the same, K % 4 == 1", ("conv32", 3, 1), 103, K=17, **FIRST),
    # M = 70 and 48: below 128 rows there is one split and no reduce launch
    _conv("s2_9x13", "3x3 / s2 / pad 1, 9x13 -> 5x7: OW < 16 (row wraps and an image wrap inside a step), ragged last step, C % 128 != 0",
          ("conv128", 1, 0), 104, N=2, H=9, W=13, C=48, K=72, R=3, stride=2, pad=1),
    _conv("s2_8x12", "3x3 / s2 / pad 1, 8x12 -> 4x6: even sizes, the last input row and column are never the centre",
          ("conv128", 1, 0), 105, N=2, H=8, W=12, C=48, K=72, R=3, stride=2, pad=1),
    _conv("s2_1x1", "1x1 / s2 / pad 0 on 9x13: two k tiles; the stride keeps it off the TN route", ("conv128", 1, 0), 106,
          N=2, H=9, W=13, C=64, K=256, stride=2),
    # M = 442: cap 4 -> rows ceil(111 / 16) * 16 = 112 -> 4 splits; M = 720: cap 6 -> 128 rows -> 6; M = 512: 4 of 128
    _conv("dil2", "3x3 dilated by 2 on 13x17", ("conv64", 4, 1), 107, N=2, H=13, W=17, C=64, K=48, R=3, dil=2, pad=2),
    _conv("dil12", "3x3 dilated by 12 on 20x18: partly dead taps", ("conv64", 6, 1), 108, N=2, H=20, W=18, C=64, K=48, R=3, dil=12, pad=12),
    _conv("dil36", "3x3 dilated by 36 on 16x16: only the centre tap is live, the eight other slabs are exact zeros", ("conv64", 4, 1), 109,
          N=2, H=16, W=16, C=64, K=48, R=3, dil=36, pad=36),
    # M = 180: cap 2 -> rows ceil(90 / 16) * 16 = 96 -> 2 splits
    _conv("valid3x3", "3x3 / pad 0 (valid convolution), K == 32: the 32-row tile full", ("conv32", 2, 1), 110, N=2, H=11, W=12, C=32, K=32, R=3),
    _conv("c304", "1x1, C = 304: three c tiles, the last 48 wide; small M", ("conv32", 1, 0), 111, N=2, H=5, W=9, C=304, K=19),
    # M = 220: cap 2 -> rows 112 -> 2 splits
    _conv("x_slice", "x as a channel slice (ldx 96, c0 32)", ("conv32", 2, 1), 112, N=2, H=10, W=11, C=32, K=24, R=3, pad=1, ldx=96, x_c0=32),
    _conv("padded_dwp", "raw call with Kpad = K + 8 and Cp = C + 12: the padding rows and columns are written as zeros", ("conv32", 3, 1), 113,
          K=19, Kpad=27, Cp=44, **FIRST),
    _conv("affine_relu", "shared affine + ReLU", ("conv32", 3, 1), 114, K=19, affine="shared", relu=True, **FIRST),
    _conv("affine_only", "affine without ReLU", ("conv32", 3, 1), 115, K=19, affine="shared", **FIRST),
    _conv("relu_only", "ReLU without an affine", ("conv32", 3, 1), 116, K=19, relu=True, **FIRST),
    # M = 546: cap 5 -> rows ceil(110 / 16) * 16 = 112 -> 5 splits at 112, 224, 336, 448; images end at 182 and 364
    _conv("per_sample", "per-sample affine (the Dropout2d fold) + ReLU, N = 3, split boundaries inside images", ("conv32", 5, 1), 117,
          K=19, affine="per_sample", relu=True, **dict(FIRST, N=3)),
    _conv("m1", "one output pixel", ("conv32", 1, 0), 118, N=1, H=1, W=1, C=32, K=19, R=3, pad=1),
    _conv("m16", "16 output pixels in two images: exactly one step", ("conv32", 1, 0), 119, N=2, H=2, W=4, C=32, K=19, R=3, pad=1),
    _conv("m17", "17 output pixels: one step and one pixel", ("conv32", 1, 0), 120, N=1, H=1, W=17, C=32, K=19, R=3, pad=1),
    # ---- C2: the reducers through real calls ----------------------------------------------------------------------------------
    # 2 c tiles x 9 taps = 18 jobs per split, cap ceil(2179 / 128) = 18 -> 18 splits of 128 (the last: 3 rows); slab4 = 9 * 128 * 256 / 4
    # = 73728 >= 65536: sequential, two 8-deep passes (splits 1..16) and one split left
    _conv("seq_large_slab", "sequential reducer because the slab is large: 18 splits", ("conv128", 18, 1), 121,
          N=1, H=1, W=2179, C=256, K=128, R=3, pad=1),
] + [
    # 1x1, C = 64 (C % 128 != 0 keeps it off the narrow kernel), K = 19: one job per split, so splits = ceil(M / 128); M = 128 * splits
    # - 5 leaves the last step of the last split ragged. slab4 = 20 * 64 / 4 = 320.
    _conv(f"par_g{G}_s{sp}", f"parallel reducer, G = {G}, {sp} splits: " + ("splits % 4G == 0" if sp % (4 * G) == 0 else "a remainder after the 4-deep passes"),
          ("conv32", sp, G), 130 + sp, N=1, H=1, W=128 * sp - 5, C=64, K=19)
    for sp, G in ((8, 2), (13, 2), (16, 4), (27, 4), (32, 8), (53, 8), (64, 16), (101, 16), (128, 32), (257, 32))
] + [
    # ---- C3: one case per remaining class -------------------------------------------------------------------------------------
    # one c tile: min(3072 or 2048, ceil(16387 / 512) = 33) -> rows ceil(497 / 2) * 2 = 498 -> 33 splits; slab4 = 20 * 128 / 4 = 640 (K = 19),
    # 1536 (K = 48): G doubles while splits >= 8 G -> 8
    _conv("narrow_k19", "gemm_tn_narrow_kernel, 32-row tile", ("narrow", 33, 8), 401, N=1, H=1, W=16387, C=128, K=19, ref="device"),
    _conv("narrow_k19_affine", "the same with affine + ReLU", ("narrow", 33, 8), 402, N=1, H=1, W=16387, C=128, K=19, affine="shared", relu=True, ref="device"),
    _conv("narrow_k48", "gemm_tn_narrow_kernel, 64-row tile (float2 loads of dy)", ("narrow", 33, 8), 403, N=1, H=1, W=16387, C=128, K=48, ref="device"),
    _conv("narrow_k48_affine", "the same with affine + ReLU", ("narrow", 33, 8), 404, N=1, H=1, W=16387, C=128, K=48, affine="shared", relu=True, ref="device"),
    # one tile (two for K = 136): the one-wave plan has 2 jobs, far below 768, so the LDS kernel; cap ceil(300 / 128) = 3 -> rows
    # ceil(100 / 16) * 16 = 112 -> 3 splits
    _conv("tn_lds_k128", "gemm_tn_wgrad_kernel, one position", ("tn_lds", 3, 1), 405, N=1, H=15, W=20, C=128, K=128, ref="device"),
    _conv("tn_lds_k136", "the same, K % 128 != 0: a second k tile of 8 rows", ("tn_lds", 3, 1), 406, N=1, H=15, W=20, C=128, K=136, ref="device"),
    # 64 positions x 2 k tiles x 8 wide c tiles = 1024 jobs = two full rounds of 512, 40 rows: no split
    _conv("tn_wide", "gemm_tn2_wgrad_kernel: 1024 wide tiles, no split", ("tn_wide", 1, 0), 407, batch=64, T=40, C=2048, K=136, ref="device"),
    # 48 x 4 x 4 = 768 one-wave jobs = 3/4 of the SIMDs, 64 rows: no split
    _conv("tn_direct", "gemm_tn_direct_kernel: 768 one-wave jobs", ("tn_direct", 1, 0), 408, batch=48, T=64, C=512, K=512, ref="device"),
    # forced (a single position reaches the kernel by default only from 192 splits of 256 rows x 4 tiles: 50 MB of x): one tile,
    # cap ceil(1000 / 256) = 4 -> 4 splits of 250 rows
    _conv("tn_direct_rows", "gemm_tn_direct_kernel, one position: row splits and a sliced dy (MSS_WGRAD_TN=7)", ("tn_direct", 4, 1), 409,
          N=1, H=25, W=40, C=128, K=128, lddy=160, dy_c0=32, env={"MSS_WGRAD_TN": "7"}, ref="device"),
    # 65 x 16 = 1040 tiles = 1024 whole + 16 tail tiles; 1024 / 16 = 64 ranges wanted, ceil(300 / 256) = 2 possible
    Case("tn_direct_tail", "gemm_tn_direct_kernel with the tail plan: 1024 whole tiles + 16 x 2", dict(kernel="tn_direct_tail", splits=2, reduce_group=0, full=1024),
         410, batch=65, T=300, C=512, K=512, ref="device"),
    # 36 positions x 3 images (the rows of tests/test_gpu_aspp_wgrad_packed.py's 200-row case, with 512 columns so that extents differ
    # in whole tiles): extents 16 * (8 + k_steps) = 512, 176, 304 columns -> 4, 2, 3 of the 4 c tiles are written
    Case("tn_direct_perimg", "per-image form: zeros behind an extent inside a tile, tiles behind it unwritten", dict(kernel="tn_direct_perimg", splits=1, reduce_group=0),
         411, batch=108, T=200, C=512, K=256, k_base=8, k_steps=(24, 3, 11), ref="device"),
    # 32 x 2 k tiles x 2 wide c tiles = 128 jobs per split; floor(520 / 256) = 2 splits -> 256 jobs, the least it takes; rows
    # ceil(260 / 16) * 16 = 272, and 520 % 16 != 0: the masked kernel with the last split shifted back. slab4 = 32 * 256 * 512 / 4
    Case("tn_bf16x3", "the split-bf16 TN kernel at its smallest eligible size, rows % 16 != 0", dict(kernel="tn_bf16x3", splits=2, reduce_group=1),
         412, batch=32, T=520, C=512, K=256, route=1, ref="device"),
] + [
    # K = 128 + 32 over 16385 rows. First part (K = 128, a row stride on dy, 65 one-wave jobs at most): conv_wgrad_kernel, one job per
    # split, cap ceil(16385 / 128) = 129 -> 128 rows -> 129 splits (the last: one row); slab4 = 128 * 128 / 4 = 4096 -> G = 16
    # (4096 * 16 = 65536 stops the doubling). Second part: the narrow kernel as above, slab4 = 32 * 128 / 4 = 1024 -> G = 8.
    Case(f"two_part{tag}", f"K = 128 + 32: two launches, {what} dy", dict(kernel="two_part", splits=1, reduce_group=0, wide_K=128,
                                                                          parts=[("conv128", 129, 16), ("narrow", 33, 8)]),
         420 + ld, N=1, H=1, W=16385, C=128, K=160, lddy=ld, dy_c0=c0, ref="device")
    for tag, what, ld, c0 in (("", "dense", 0, 0), ("_sliced", "sliced", 256, 64))
]

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def conv_args(c, x, scale=None, shift=None, k_steps=None, gap=0):
    """MssConvArgs of a case. x, scale, shift, k_steps: addresses (ints) of the first element the call may touch; gap: NaN rows
    between the positions of a batched case (they enter the batch strides)."""
    from multishiftseg_amd._lib import MssConvArgs
    a = MssConvArgs()
    a.x = x
    a.N, a.H, a.W, a.C, a.ldx = c.N, c.H, c.W, c.C, c.ldx
    a.OH, a.OW, a.K, a.Kpad = c.OH, c.OW, c.K, c.Kpad
    a.R, a.S, a.stride, a.dil, a.pad = c.R, c.R, c.stride, c.dil, c.pad
    if c.affine:
        a.in_scale, a.in_shift = scale, shift
        a.in_ss_stride = c.C if c.affine == "per_sample" else 0
    a.in_relu = int(c.relu)
    a.route = c.route
    if c.batch:
        a.batch, a.x_bs, a.y_bs = c.batch, (c.T + gap) * c.ldx, (c.T + gap) * c.lddy
    if c.k_steps:
        a.k_steps, a.k_base, a.k_imgs = k_steps, c.k_base, len(c.k_steps)
    return a


def answered_plan(c, a, dy, dwp, ws_bytes):
    """What mss_conv2d_wgrad_plan answers for the case, in the form of Case.expect (only its keys), and the whole answer."""
    import ctypes
    from multishiftseg_amd import _lib

    def ask(part):
        pl = _lib.MssWgradPlan()
        rc = _lib.value("mss_conv2d_wgrad_plan", ctypes.byref(a), dy, c.lddy, dwp, c.Cp, ws_bytes, part, ctypes.byref(pl))
        assert rc == 0, (c.name, part, rc)
        return pl
    pl = ask(0)
    got = {"kernel": KERNELS[pl.kernel], "splits": pl.splits, "reduce_group": pl.reduce_group, "full": pl.full, "wide_K": pl.wide_K}
    if pl.kernel == KERNELS.index("two_part"):
        got["parts"] = [(KERNELS[q.kernel], q.splits, q.reduce_group) for q in (ask(1), ask(2))]
    return {k: got.get(k) for k in c.expect}, pl
