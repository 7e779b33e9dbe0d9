"""The one case table of the exact forward tests: tests/test_fwd_exact_cpu.py (expected plans through tests/fwd_route_check.cpp,
exactness condition, plane shares, reference, sensitivity; no GPU) and tests/test_gpu_fwd_exact.py (every case through one raw
mss_conv2d_forward_f32 call, equality with float64).

Two data classes (tests/ref_fwd.py has the reference of each):
  "int"     x and w integers in [-2, 2], prologue / epilogue scales in {0.5, 1, 2}, shifts in {1, 2} (positive: an activated padding
            tap would be non-zero), epilogue shifts and residuals integers in [-2, 2]; on rows with statistics [-1, 1] and {0.5, 1},
            because a statistics sum holds 64 squares of outputs. Every term is a multiple of 1/4 far below
            2^24 of them, so fp32 is exact in any summation order; for the split kernels such values are one bf16 term and two zeros.
  "planes"  split routes only: values +-(1 + 2^-9 + 2^-18) (hi, mid and lo all non-zero; no round-to-even tie anywhere in the split),
            some +-(1 + 2^-9) and +-1, and exact zeros. The six kept products then have the granule 2^-18 and a full product the
            magnitude 1, so for a ratio of at most 2^20 an output may hold at most THREE non-zero products. Random sparsity cannot
            promise that, so the zeros follow a pattern: x is non-zero on the even channels and on ONE odd channel per pixel (3x3: per
            pixel with y % 3 == x % 3 == 0, of which a dilation that is no multiple of 3 puts at most one under a filter), w on the
            odd channels and on ONE even (tap, channel) per output channel. Every output is then the sum of at most two full
            three-plane products, every non-zero element of either operand meets a non-zero partner in some output, and more than a
            quarter of the elements of x and of w have each plane non-zero. With a prologue the activated values are the lattice
            values (all positive, x = (value - shift) / scale exactly, scale in {1, 2}, shift in {1, 2}) and the zeros are x = -2,
            which the ReLU removes.

A row's `expect` is the plan derived by hand from csrc/fwd_route.h and csrc/gemm_rounds.h; test_fwd_exact_cpu.py compares it with
what the stand-alone checker prints for the row, so a wrong derivation fails there instead of quietly testing another kernel. The rules:
  conv_igemm: K <= 64: 256 x 64 x 16; else 128 x 128 x 16 (x 32 for C >= 2048, C % 32 == 0, K <= 256); mtiles = ceil(M / BM),
    ntiles = ceil(K / BN); per_sample = per-sample affine and OH * OW % BM != 0.
  few_rows: 1x1, nothing fused, M <= 32: the bucket 8 / 16 / 32.
  GEMM kernels (1x1 / stride 1, K > 64, or 32 <= K <= 64 with C >= 48 and M >= 16384): mtiles = ceil(M / 128); 128-wide tiles
    ntiles = ceil(K / 128); wide (256) needs K % 256 == 0, C >= 256 and tiles256 = mtiles * K / 256 * batch >= 1024 with the last of
    its rounds of 512 at least 0.8 full (or the narrow tiles' last round of 768 no more than 0.15 fuller); hybrid = wide tiles
    [0, full) + narrow for the rest: (a) wide, one position, full <= 2048, 0 < rem <= 384 (MSS_GEMM_TAIL=1: any batch); (b) not
    wide, one position, 512 < tiles256 < 1024, rem <= 384. variant 3 needs C >= 48.
  split GEMM: the width rule alone; mfma 16 needs no prologue, K % 4 == 0, ldy % 4 == 0 and y on the 16-byte grid.
  split implicit GEMM: wide from 1024 wide tiles, K % 256 == 0; always mfma 32."""
from dataclasses import dataclass, field

import torch

from ref_fwd import out_size

NARROW, WIDE, HYBRID = 0, 1, 2
CODES = {"conv_igemm": 0, "gemm_nt": 1, "gemm_nt_perimg": 1, "few_rows": 2, "gemm_nt_bf16x3": 3, "conv_bf16x3": 4, "rowaff_bf16x3": 4}
GUARD = 3           # NaN rows before, behind and between batch entries (they enter the batch strides)
PLAN_KEYS = ("kernel", "BM", "BN", "BK", "variant", "affine", "per_sample", "mfma", "mode", "full", "rem", "mtiles", "ntiles")
V3, V2, V1 = 1.0 + 2.0 ** -9 + 2.0 ** -18, 1.0 + 2.0 ** -9, 1.0


@dataclass
class Case:
    name: str
    intent: str
    expect: dict                    # PLAN_KEYS
    seed: int
    N: int = 1                      # images per batch entry; x [N][H][W][C] (a GEMM: H = 1, W = rows per image)
    H: int = 1
    W: int = 1
    C: int = 32
    K: int = 128
    R: int = 1
    stride: int = 1
    dil: int = 1
    batch: int = 0                  # > 1: that many products, GUARD NaN rows between their x and between their y
    ldx: int = 0                    # pixel stride of x (0: C) and the first channel of the slice
    x_c0: int = 0
    ldy: int = 0                    # the same for y (0: K) -- and for res, which lives in a buffer of y's shape
    y_c0: int = 0
    affine: str = ""                # "", "shared", "per_sample": the prologue, always with ReLU
    out_affine: bool = False
    out_relu: bool = False
    res: str = ""                   # "", "add", "mask"
    stats: bool = False
    split: bool = False             # MssConvArgs.w_split set
    k_steps: tuple = ()             # per-image reduction lengths: of the N images, or with k_imgs of the images b % len(k_steps)
    k_imgs: bool = False
    k_base: int = 0
    env: dict = field(default_factory=dict)     # MSS_GEMM* switches
    data: str = "int"
    ref: str = "cpu"                # "cpu": ref_fwd on the CPU; "device": float64 matrix products on the device (1x1 / stride 1)

    def __post_init__(self):
        self.pad = self.dil * (self.R // 2)
        self.ldx = self.ldx or self.C
        self.ldy = self.ldy or self.K
        self.Kpad = 64 if self.K <= 64 else (self.K + 127) // 128 * 128            # mss_conv2d_kpad
        self.OH = out_size(self.H, self.R, self.stride, self.dil, self.pad)
        self.OW = out_size(self.W, self.R, self.stride, self.dil, self.pad)
        self.M = self.N * self.OH * self.OW
        self.nb = max(self.batch, 1)
        self.nw = self.nb if self.batch > 1 else (self.N if self.k_steps else 1)   # weight sets: per entry, or per image (one-batch form)
        self.gemm = self.R == 1 and self.stride == 1
        assert self.data == "int" or self.split
        assert not (self.stats and self.data == "planes")      # squares of lattice values leave the granule

    @property
    def geometry(self):
        """What the reference and sensitivity checks of the CPU test run on."""
        return self.ref == "cpu" and self.batch <= 1 and not self.k_steps

    @property
    def wrapper(self):
        """kernels.conv2d can express the case: one product, channel offsets on the 16-byte grid, no forcing switch. Not the
        three-plane rows whose K leaves a tail of at most 64 channels: the wrapper runs that tail on the native fp32 kernel, which
        computes the true product and not the six kept ones."""
        tail = self.K > 128 and 0 < self.K % 128 <= 64
        return self.batch <= 1 and not self.k_steps and self.y_c0 % 4 == 0 and self.ldy % 4 == 0 and not self.env and not (self.data == "planes" and tail)

    @property
    def y_misalign(self):
        """Bytes between y's first element and the 16-byte grid (the buffer itself is aligned, GUARD rows precede the data)."""
        return 4 * (GUARD * self.ldy + self.y_c0) % 16

    def extents(self):
        """Per batch entry and image: the channels of x that exist (per-image forms), else C."""
        if not self.k_steps:
            return [[self.C] * self.N for _ in range(self.nb)]
        if self.k_imgs:
            return [[16 * (self.k_base + self.k_steps[b % len(self.k_steps)])] for b in range(self.nb)]
        return [[16 * s for s in self.k_steps]]

    def checker_line(self):
        """The row in the column format of tests/fwd_route_check.cpp."""
        sw = {"MSS_GEMM": 1, "MSS_GEMM_VARIANT": 3, "MSS_GEMM_TAIL": -1, "MSS_GEMM_SPLIT_MFMA": 16}
        sw.update({k: int(v) for k, v in self.env.items() if k in sw})
        x_bs = (self.M + GUARD) * self.ldx if self.batch > 1 else 0
        cols = [self.N, self.H, self.W, self.C, self.ldx, self.K, self.Kpad, self.ldy, self.R, self.stride, self.dil, self.batch, x_bs, 0,
                int(bool(self.affine)), self.C if self.affine == "per_sample" else 0, int(self.out_affine or self.out_relu), int(bool(self.res)),
                int(self.stats), int(self.split), self.y_misalign, int(bool(self.k_steps)), len(self.k_steps) if self.k_imgs else 0, self.k_base,
                self.Kpad * self.C if self.k_steps and not self.k_imgs else 0] + list(sw.values())
        return " ".join(map(str, cols))


def _plane_values(g, shape, positive):
    u = torch.randint(0, 8, shape, generator=g)
    v = torch.where(u < 6, torch.tensor(V3, dtype=torch.float64), torch.where(u == 6, torch.tensor(V2, dtype=torch.float64), torch.tensor(V1, dtype=torch.float64)))
    return v if positive else v * (2 * torch.randint(0, 2, shape, generator=g) - 1).double()


def operands(c):
    """The case's data on the CPU, float32 and exactly on its lattice: x [nb][N][H][W][C], w [nw][K][C][R][R], scale / shift ([C] or
    [N][C]), out_scale / out_shift [K], res [nb][M][K] (each None where the case has none)."""
    g = torch.Generator().manual_seed(c.seed)
    C, K, R, taps = c.C, c.K, c.R, c.R * c.R

    top = 1 if c.stats else 2           # rows with statistics: the sums of 64 squares must hold the condition too

    def ints(*shape):
        return torch.randint(-top, top + 1, shape, generator=g).float()
    scales = torch.tensor([0.5, 1.0] if c.stats else [0.5, 1.0, 2.0])
    scale = shift = None
    ashape = (c.N, C) if c.affine == "per_sample" else (C,)
    if c.data == "int":
        x, w = ints(c.nb, c.N, c.H, c.W, C), ints(c.nw, K, C, R, R)
        if c.affine:
            scale = scales[torch.randint(0, len(scales), ashape, generator=g)]
            shift = torch.randint(1, 3, ashape, generator=g).float()
    else:
        half = C // 2
        ch = torch.arange(C)
        b, n, h, wd = torch.meshgrid(torch.arange(c.nb), torch.arange(c.N), torch.arange(c.H), torch.arange(c.W), indexing="ij")
        if R == 1:
            which, has = (b + n + h * c.W + wd) % half, torch.ones_like(b, dtype=torch.bool)
        else:
            assert c.dil % 3 != 0
            which, has = (n + h // 3 + wd // 3) % half, (h % 3 == 0) & (wd % 3 == 0)
        live = (ch % 2 == 0) | (has[..., None] & (ch // 2 == which[..., None]))
        target = torch.where(live, _plane_values(g, live.shape, bool(c.affine)), torch.zeros((), dtype=torch.float64))
        k, cc, r, s = torch.meshgrid(torch.arange(K), ch, torch.arange(R), torch.arange(R), indexing="ij")
        wlive = (cc % 2 == 1) | ((r * R + s) * half + cc // 2 == k % (taps * half))
        w = torch.where(wlive, _plane_values(g, wlive.shape, False), torch.zeros((), dtype=torch.float64)).float()[None].repeat(c.nw, 1, 1, 1, 1)
        if c.nw > 1:
            w = w * (2 * torch.randint(0, 2, w.shape, generator=g) - 1).float()
        if c.affine:
            scale = torch.randint(1, 3, ashape, generator=g).float()
            shift = torch.randint(1, 3, ashape, generator=g).float()
            sc = scale.double().view((1, c.N, 1, 1, C) if scale.dim() == 2 else (1, 1, 1, 1, C))
            sh = shift.double().view(sc.shape)
            target = torch.where(live, (target - sh) / sc, torch.full((), -2.0, dtype=torch.float64))
        x = target.float()
        assert torch.equal(x.double(), target)
    osc = osh = res = None
    if c.out_affine:
        osc, osh = scales[torch.randint(0, len(scales), (K,), generator=g)], ints(K)
    if c.res:
        res = ints(c.nb, c.M, K)
    return dict(x=x, w=w, scale=scale, shift=shift, out_scale=osc, out_shift=osh, res=res)


def _plan(kernel, BM=0, BN=0, BK=0, variant=0, affine=0, per_sample=0, mfma=0, mode=NARROW, full=0, rem=0, mtiles=0, ntiles=0):
    return dict(kernel=kernel, BM=BM, BN=BN, BK=BK, variant=variant, affine=affine, per_sample=per_sample, mfma=mfma, mode=mode, full=full,
                rem=rem, mtiles=mtiles, ntiles=ntiles)


def _ig(BM, BN, BK, mtiles, ntiles, affine=0, per_sample=0):
    return _plan("conv_igemm", BM, BN, BK, affine=affine, per_sample=per_sample, mtiles=mtiles, ntiles=ntiles)


def _nt(BN, variant, mtiles, ntiles, affine=0, mode=NARROW, full=0, rem=0, kernel="gemm_nt"):
    return _plan(kernel, BN=BN, variant=variant, affine=affine, mode=mode, full=full, rem=rem, mtiles=mtiles, ntiles=ntiles)


def _sp(kernel, BN, mfma, mtiles, ntiles, affine=0, per_sample=0):
    return _plan(kernel, BN=BN, mfma=mfma, affine=affine, per_sample=per_sample, mode=WIDE if BN == 256 else NARROW, mtiles=mtiles, ntiles=ntiles)


EPI = dict(out_affine=True, out_relu=True, stats=True)       # + res, a window and a slice where a row says so
BIG = dict(H=1, C=256, K=4096, ref="device")                 # 16 column tiles of 256: 64 row tiles are 1024 wide tiles


def _both(name, intent, expect, seed, **kw):
    """A split-route row in both data classes."""
    return [Case(name + "_int", intent + " (integer lattice)", expect, seed, split=True, **kw),
            Case(name + "_planes", intent + " (three-plane lattice)", expect, seed + 1, split=True, data="planes", **kw)]


CASES = [
    # ---- conv_igemm_kernel ----------------------------------------------------------------------------------------------------
    Case("ig64_k1_m255", "256x64x16, one output channel, one K-step (C = 16), M = BM - 1", _ig(256, 64, 16, 1, 1), 101, H=15, W=17, C=16, K=1, R=3),
    Case("ig64_k63_m257", "256x64x16, K = 63, two K-steps per tap (C = 32), M = BM + 1 on a one-row image", _ig(256, 64, 16, 2, 1), 102, H=1, W=257, C=32, K=63, R=3),
    Case("ig64_k64_m512", "256x64x16, K = 64, M = 2 BM: whole tiles, full epilogue with statistics groups of 64 rows", _ig(256, 64, 16, 2, 1), 103,
         N=2, H=16, W=16, C=16, K=64, R=3, res="add", ldy=80, y_c0=12, **EPI),
    Case("ig128_k65_m129", "128x128x16, K = 65, M = BM + 1", _ig(128, 128, 16, 2, 1), 104, H=3, W=43, C=16, K=65, R=3),
    Case("ig128_k129_m127", "128x128x16, K = 129: a second column tile of one channel, M = BM - 1", _ig(128, 128, 16, 1, 2), 105, H=1, W=127, C=32, K=129, R=3),
    Case("ig128_k200_affine", "128x128x16, K = 200, M = 2 BM, prologue affine + ReLU with positive shifts: padding taps must stay zero",
         _ig(128, 128, 16, 2, 2, affine=1), 106, H=16, W=16, C=32, K=200, R=3, affine="shared"),
    Case("ig128x32_dil2", "128x128x32 (C = 2048, K <= 256), 3x3 dilated by 2 on 9x11", _ig(128, 128, 32, 1, 1), 107, H=9, W=11, C=2048, K=128, R=3, dil=2),
    Case("ig_s2_9x13", "3x3 / stride 2 on odd sizes, 9x13 -> 5x7", _ig(128, 128, 16, 1, 1), 108, N=2, H=9, W=13, C=32, K=72, R=3, stride=2),
    Case("ig_s2_8x12", "3x3 / stride 2 on even sizes, 8x12 -> 4x6: the last input row and column are never the centre", _ig(128, 128, 16, 1, 1), 109,
         N=2, H=8, W=12, C=32, K=72, R=3, stride=2),
    Case("ig_dil20", "3x3 dilated by 20 on 16x16: only the centre tap is live", _ig(256, 64, 16, 2, 1), 110, N=2, H=16, W=16, C=32, K=48, R=3, dil=20),
    Case("ig_1x1_s2", "1x1 / stride 2 on 9x13: the stride keeps it off the GEMM kernels", _ig(128, 128, 16, 1, 1), 111, N=2, H=9, W=13, C=64, K=128, stride=2),
    Case("ig_per_sample_3img", "per-sample affine, N = 3 with OH * OW = 42 < BM / 2: one tile holds three images", _ig(128, 128, 16, 1, 1, affine=1, per_sample=1), 112,
         N=3, H=6, W=7, C=32, K=128, R=3, affine="per_sample"),
    Case("ig_per_sample_whole", "per-sample affine with OH * OW = BM: no tile straddles, the shared-affine instantiation", _ig(128, 128, 16, 2, 1, affine=1), 113,
         N=2, H=8, W=16, C=32, K=128, R=3, affine="per_sample"),
    Case("ig64_below_16384_rows", "a 1x1 / stride-1 product of 48 channels one row short of the 128x64 GEMM tile's threshold", _ig(256, 64, 16, 64, 1), 117,
         W=16383, C=64, K=48, ref="device"),
    Case("ig128_epi_add", "128x128x16 full epilogue: affine, ReLU, residual added, statistics with a last group of 58 rows, output window, x slice",
         _ig(128, 128, 16, 4, 2, affine=1), 114, N=2, H=13, W=17, C=32, K=200, R=3, affine="shared", res="add", ldy=216, y_c0=8, ldx=64, x_c0=16, **EPI),
    Case("ig128_epi_mask", "128x128x16, the residual gates", _ig(128, 128, 16, 4, 2), 115, N=2, H=13, W=17, C=32, K=200, R=3, res="mask", out_affine=True, stats=True),
    Case("ig64_epi_mask", "256x64x16, the residual gates, K = 48 in a window", _ig(256, 64, 16, 2, 1), 116, N=2, H=13, W=17, C=32, K=48, R=3, res="mask", ldy=64, y_c0=4, **EPI),
] + [
    # ---- gemm_few_rows_kernel: x a slice of a wider buffer throughout -----------------------------------------------------------
    Case(f"few_m{M}_k{K}", f"few rows: M = {M} (bucket {bm}), K = {K}, ldx > C", _plan("few_rows", BM=bm), 200 + M, W=M, C=C, K=K, ldx=C + 16, x_c0=8, ldy=ldy, y_c0=y0)
    for M, K, C, bm, ldy, y0 in ((1, 1, 64, 8, 0, 0), (8, 19, 528, 8, 0, 0), (9, 100, 64, 16, 104, 4), (16, 1, 64, 16, 4, 2), (17, 19, 528, 32, 0, 0), (32, 100, 64, 32, 0, 0))
] + [
    # ---- gemm_nt_kernel ---------------------------------------------------------------------------------------------------------
    Case("nt64_m16384", "128x64 tile, M = 16384: whole tiles", _nt(64, 3, 128, 1), 301, W=16384, C=64, K=48, ref="device"),
    Case("nt64_m16385", "128x64 tile, M = 16385: a last tile of one row; K = 33", _nt(64, 3, 129, 1), 302, W=16385, C=48, K=33, ldy=36, ref="device"),
    Case("nt128_v2_c32", "BN 128, variant 2 by shape (C = 32: two K-steps), M % 128 = 1", _nt(128, 2, 3, 1), 303, W=257, C=32, K=128),
    Case("nt128_v3_k200", "BN 128, variant 3, K = 200, M % 128 = 127, shared affine", _nt(128, 3, 3, 2, affine=1), 304, W=383, C=64, K=200, affine="shared"),
    Case("nt128_k65", "BN 128, K = 65", _nt(128, 3, 2, 1), 305, W=129, C=48, K=65, ldy=68),
    Case("nt128_k129", "BN 128, K = 129: a second column tile of one channel", _nt(128, 3, 2, 2), 306, W=255, C=48, K=129, ldy=132),
    Case("nt128_v2_forced", "MSS_GEMM_VARIANT=2 on a variant-3 shape", _nt(128, 2, 3, 2), 307, W=300, C=64, K=136, env={"MSS_GEMM_VARIANT": "2"}),
    Case("nt128_batch3", "batch = 3 with guard rows between the entries: x_bs and y_bs exceed the entry", _nt(128, 3, 3, 1), 308, W=257, C=48, K=128, batch=3),
    Case("nt128_per_sample", "per-sample affine on whole tiles: 3 images of 256 rows", _nt(128, 3, 6, 1, affine=1), 309, N=3, W=256, C=64, K=128, affine="per_sample"),
    Case("nt128_epi_add", "BN 128 full epilogue: affine, ReLU, residual added, statistics with a last group of 63 rows, window, x slice",
         _nt(128, 3, 3, 2, affine=1), 310, W=383, C=64, K=200, affine="shared", res="add", ldy=216, y_c0=8, ldx=96, x_c0=16, **EPI),
    Case("nt128_epi_mask", "BN 128, the residual gates", _nt(128, 3, 3, 2), 311, W=383, C=64, K=200, res="mask", out_affine=True, stats=True),
    Case("nt64_epi", "128x64 tile, full epilogue", _nt(64, 3, 129, 1, affine=1), 312, W=16385, C=64, K=48, affine="shared", res="add", ldy=64, y_c0=8, ref="device", **EPI),
    # 64 x 16 = 1024 wide tiles: two whole rounds of 512
    Case("nt256_wide", "BN 256 wide, variant 3: 1024 wide tiles", _nt(256, 3, 64, 16, mode=WIDE), 313, W=8192, **BIG),
    Case("nt256_wide_v2_epi", "BN 256 wide, variant 2 forced, full epilogue", _nt(256, 2, 64, 16, affine=1, mode=WIDE), 314, W=8192, affine="shared", res="add",
         env={"MSS_GEMM_VARIANT": "2"}, **EPI, **BIG),
    Case("nt256_group_m", "BN 256 wide with MSS_GEMM_GROUP_M=4: the grouped tile order", _nt(256, 3, 64, 16, mode=WIDE), 315, W=8192, env={"MSS_GEMM_GROUP_M": "4"}, **BIG),
    # 80 x 16 = 1280 wide tiles = 2.5 rounds, fill 0.83: wide, and the last round (256 <= 384) goes narrow; M % 128 = 1
    Case("nt256_hybrid_last_round", "hybrid rule (a): a partial last round; 1024 wide + 512 narrow tiles", _nt(256, 3, 80, 16, mode=HYBRID, full=1024, rem=256), 316,
         W=10113, **BIG),
    # 36 x 16 = 576 wide tiles = 512 + 64
    Case("nt256_hybrid_between", "hybrid rule (b): between one and two rounds; 512 wide + 128 narrow tiles, M % 128 = 123", _nt(256, 3, 36, 16, mode=HYBRID, full=512, rem=64),
         317, W=4603, **BIG),
    Case("nt_tail0", "MSS_GEMM_TAIL=0 on the same shape: all narrow", _nt(128, 3, 36, 32), 318, W=4603, env={"MSS_GEMM_TAIL": "0"}, **BIG),
    # 2 x 40 x 16 = 1280 wide tiles: a batched product is wide by default and a hybrid only with MSS_GEMM_TAIL=1
    Case("nt_tail1_batched", "MSS_GEMM_TAIL=1: a batched hybrid, the narrow launch starts inside the second entry", _nt(256, 3, 40, 16, mode=HYBRID, full=1024, rem=256), 319,
         W=5120, batch=2, env={"MSS_GEMM_TAIL": "1"}, **BIG),
    # ---- the per-image form ---------------------------------------------------------------------------------------------------
    Case("perimg128", "one-batch form, BN 128: 3 images of one tile, 3 / 8 / 5 K-steps, NaN behind each extent", _nt(128, 3, 3, 1, kernel="gemm_nt_perimg"), 401,
         N=3, W=128, C=128, K=128, k_steps=(3, 8, 5), ref="device"),
    Case("perimg256", "one-batch form, BN 256: 2 images of 32 tiles", _nt(256, 3, 64, 16, mode=WIDE, kernel="gemm_nt_perimg"), 402, N=2, W=4096, k_steps=(16, 3), **BIG),
    Case("k_imgs128", "k_imgs form, BN 128: 4 entries of 200 rows, k_base = 1", _nt(128, 3, 2, 1, kernel="gemm_nt_perimg"), 403, W=200, C=96, K=128, batch=4,
         k_steps=(3, 5), k_imgs=True, k_base=1, ref="device"),
    Case("k_imgs256", "k_imgs form, BN 256: 8 x 8 x 16 = 1024 wide tiles, k_base = 2", _nt(256, 3, 8, 16, mode=WIDE, kernel="gemm_nt_perimg"), 404, W=1000, batch=8,
         k_steps=(3, 14), k_imgs=True, k_base=2, **BIG),
] + (
    # ---- gemm_nt_bf16x3_kernel, GEMM form -----------------------------------------------------------------------------------------
    _both("sp128_mf16", "split GEMM BN 128 on the 16x16x32 instruction, M % 128 = 1", _sp("gemm_nt_bf16x3", 128, 16, 3, 2), 500, W=257, C=64, K=136)
    + _both("sp128_mf32_prologue", "BN 128, 32x32x16 by its prologue: the ticket order", _sp("gemm_nt_bf16x3", 128, 32, 3, 2, affine=1), 502, W=257, C=64, K=136, affine="shared")
    + _both("sp128_mf32_forced", "BN 128, MSS_GEMM_SPLIT_MFMA=32", _sp("gemm_nt_bf16x3", 128, 32, 3, 2), 504, W=257, C=64, K=136, env={"MSS_GEMM_SPLIT_MFMA": "32"})
    + _both("sp128_mf32_k134", "BN 128, K % 4 != 0 refuses the 16-byte stores, M % 128 = 127", _sp("gemm_nt_bf16x3", 128, 32, 3, 2), 506, W=383, C=48, K=134, ldy=136)
    + _both("sp128_mf32_window", "BN 128, a window 8 bytes off the 16-byte grid", _sp("gemm_nt_bf16x3", 128, 32, 3, 2), 508, W=383, C=48, K=136, ldy=144, y_c0=2)
    + _both("sp128_batch3", "BN 128 batched with guard rows between the entries", _sp("gemm_nt_bf16x3", 128, 16, 3, 1), 510, W=257, C=48, K=128, batch=3)
    + _both("sp256_mf16", "BN 256 on the 16x16x32 instruction: 1024 wide tiles", _sp("gemm_nt_bf16x3", 256, 16, 64, 16), 512, W=8192, **BIG)
    + _both("sp256_mf32", "BN 256 with a prologue: 32x32x16, the ticket order", _sp("gemm_nt_bf16x3", 256, 32, 64, 16, affine=1), 514, W=8192, affine="shared", **BIG)
    # ---- the implicit-GEMM split form ---------------------------------------------------------------------------------------------
    + _both("spc128_3x3_d2", "split implicit GEMM BN 128: 3x3 dilated by 2, affine + ReLU with positive shifts", _sp("conv_bf16x3", 128, 32, 4, 2, affine=1), 520,
            N=2, H=13, W=17, C=32, K=200, R=3, dil=2, affine="shared")
    + _both("spc128_3x3_s2", "3x3 / stride 2 dilated by 2 on 9x13, C = 16: one K-step per tap", _sp("conv_bf16x3", 128, 32, 1, 2), 522, N=2, H=9, W=13, C=16, K=136, R=3, stride=2, dil=2)
    + _both("spc128_1x1_s2", "1x1 / stride 2", _sp("conv_bf16x3", 128, 32, 1, 1), 524, N=2, H=9, W=13, C=64, K=128, stride=2)
    + _both("spc256_3x3", "BN 256: 64 x 16 = 1024 wide tiles of a 3x3 layer over 16 channels", _sp("conv_bf16x3", 256, 32, 64, 16), 526, H=64, W=128, C=16, K=4096, R=3)
    + _both("sp_rowaff", "the per-row-affine kernel: 3 images of 100 rows, tiles straddle images", _sp("rowaff_bf16x3", 128, 32, 3, 1, affine=1, per_sample=1), 528,
            N=3, W=100, C=64, K=128, affine="per_sample")
) + [
    # ---- the split kernels' epilogues (integer lattice: the statistics square the values) ----------------------------------------
    Case("sp128_mf16_epi", "split GEMM, 16x16x32 epilogue: affine, ReLU, residual added, statistics, an aligned window, x slice", _sp("gemm_nt_bf16x3", 128, 16, 3, 2), 540,
         W=383, C=64, K=200, res="add", ldy=216, y_c0=8, ldx=96, x_c0=16, split=True, **EPI),
    Case("sp128_mf32_epi_mask", "split GEMM, 32x32x16 epilogue with a prologue, the residual gates", _sp("gemm_nt_bf16x3", 128, 32, 3, 2, affine=1), 541,
         W=383, C=64, K=200, affine="shared", res="mask", ldy=216, y_c0=8, split=True, **EPI),
    Case("spc128_epi", "split implicit GEMM, full epilogue with the residual added", _sp("conv_bf16x3", 128, 32, 4, 2, affine=1), 542,
         N=2, H=13, W=17, C=32, K=200, R=3, dil=2, affine="shared", res="add", ldy=216, y_c0=8, ldx=64, x_c0=16, split=True, **EPI),
    Case("sp_rowaff_epi", "the per-row-affine kernel, full epilogue", _sp("rowaff_bf16x3", 128, 32, 3, 1, affine=1, per_sample=1), 543,
         N=3, W=100, C=64, K=128, affine="per_sample", res="add", ldy=144, y_c0=4, split=True, **EPI),
]

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES) and len({c.seed for c in CASES}) == len(CASES)


def conv_args(c, x, w, y, scale=None, shift=None, out_scale=None, out_shift=None, res=None, stats=None, w_split=None, k_steps=None):
    """MssConvArgs of a case from the addresses (ints) of the first element of each operand."""
    from multishiftseg_amd._lib import MssConvArgs
    a = MssConvArgs()
    a.x, a.w, a.y = x, w, y
    a.N, a.H, a.W, a.C, a.ldx = c.N, c.H, c.W, c.C, c.ldx
    a.OH, a.OW, a.K, a.Kpad, a.ldy = c.OH, c.OW, c.K, c.Kpad, c.ldy
    a.R, a.S, a.stride, a.dil, a.pad = c.R, c.R, c.stride, c.dil, c.pad
    if c.affine:
        a.in_scale, a.in_shift, a.in_relu = scale, shift, 1
        a.in_ss_stride = c.C if c.affine == "per_sample" else 0
    if c.out_affine:
        a.out_scale, a.out_shift = out_scale, out_shift
    a.out_relu = int(c.out_relu)
    if c.res:
        a.res, a.ldres, a.res_mask = res, c.ldy, int(c.res == "mask")
    if c.stats:
        a.stats = stats
    if c.split:
        a.w_split = w_split
    if c.batch > 1:
        a.batch, a.x_bs, a.w_bs, a.y_bs = c.batch, (c.M + GUARD) * c.ldx, c.Kpad * c.C, (c.M + GUARD) * c.ldy
    if c.k_steps:
        a.k_steps, a.k_base = k_steps, c.k_base
        if c.k_imgs:
            a.k_imgs = len(c.k_steps)
        else:
            a.w_img_stride = c.Kpad * c.C
    return a


def activated(c, ops, dev="cpu", affine_of=None):
    """act(x) in float64 on `dev`, [nb][N][H][W][C], with exact zeros behind each image's extent (per-image forms)."""
    import ref_fwd
    x = ops["x"].to(dev)
    sc, sh = (ops["scale"].to(dev), ops["shift"].to(dev)) if c.affine else (None, None)
    a = torch.stack([ref_fwd.act(x[b], sc, sh, bool(c.affine), affine_of) for b in range(c.nb)])
    for b, per_image in enumerate(c.extents()):
        for n, ext in enumerate(per_image):
            a[b, n, ..., ext:] = 0.0
    return a


def accumulators(c, ops, dev="cpu", absolute=False, wrong=None, only=None):
    """The products before the epilogue, float64 [nb][M][K] on `dev`: index arithmetic on the CPU for the geometry rows, matrix
    products for the 1x1 / stride-1 rows; on the split route the six kept products. absolute: the sum of the terms' magnitudes. wrong / only: ref_fwd.conv's, and
    wrong = ("affine", rows): image n takes the per-sample affine of row rows[n]."""
    import ref_fwd
    # the prologue and the split always on the CPU: frexp / ldexp / round are exact there, a device's float64 versions need not be
    a = activated(c, ops, "cpu", affine_of=wrong[1] if wrong and wrong[0] == "affine" else None)
    w = ops["w"].double()
    if wrong and wrong[0] == "affine":
        wrong = None
    if not c.gemm or wrong or only:
        return torch.stack([ref_fwd.product(a[b], w[b if c.batch > 1 else 0], c.split, c.stride, c.dil, c.pad, wrong, absolute, only).view(c.M, c.K) for b in range(c.nb)])
    a, w = a.view(c.nb, c.N, c.M // c.N, c.C), w.view(c.nw, c.K, c.C)
    ap = ref_fwd.split3(a) if c.split else (a,)
    wp = ref_fwd.split3(w) if c.split else (w,)
    ap, wp = [(t.abs() if absolute else t).to(dev) for t in ap], [(t.abs() if absolute else t).to(dev) for t in wp]
    # the kept products plane by plane, each an integer matrix product (ref_fwd.lattice_matmul); planes that are all zero are skipped
    kept = ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)) if c.split else ((0, 0),)
    some = [[bool(t[b].any()) for b in range(t.shape[0])] for t in ap], [[bool(t[i].any()) for i in range(t.shape[0])] for t in wp]
    out = torch.zeros((c.nb, c.N, c.M // c.N, c.K), dtype=torch.float64, device=dev)
    for b in range(c.nb):
        for n in range(c.N):
            ws = b if c.batch > 1 else (n if c.k_steps else 0)
            for i, j in kept:
                if some[0][i][b] and some[1][j][ws]:
                    out[b, n] += ref_fwd.lattice_matmul(ap[i][b, n], wp[j][ws])
    return out.view(c.nb, c.M, c.K)


def reference(c, ops, dev="cpu"):
    """(y [nb][M][K] as stored, stats [ceil(M / 64)][2][K] or None), float64 on `dev`."""
    import ref_fwd
    acc = accumulators(c, ops, dev)

    def on(t):
        return None if t is None else t.to(dev)
    y = ref_fwd.epilogue(acc, on(ops["out_scale"]), on(ops["out_shift"]), on(ops["res"]), c.res == "mask", c.out_relu)
    return y, (ref_fwd.stats(y[0]) if c.stats else None)
