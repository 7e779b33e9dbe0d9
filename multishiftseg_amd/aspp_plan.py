"""The route of the DeepLab head's ASPP block, decided once per forward from the facts of the step and readable without a GPU.

ASPP's three dilated 3x3 branches (rates d, 2d, 3d on the same 4096-channel map) can take their Winograd-domain inputs X' from one
single-read kernel, run on the trunk's two un-multiplied factors (the composed route), leave the Dropout2d-zeroed channels out (the
dropped route), share one product launch (the pair) and keep X' for the weight gradients. plan() answers all of it as an immutable
AsppPlan; deepv3.DeepWV3Plus._head_forward executes it top to bottom, `saved` carries it, and _head_backward_impl reads the route
from it. This module is the only reader of MSS_ASPP_COMPOSE, MSS_ASPP_DROPOUT_COMPACT, MSS_WINO_ASPP3 and MSS_WINO_PAIR and holds
the per-image products' offset / batch gate once. The Winograd tile policy every 3x3 layer follows (wino_tile, use_winograd) stands
here too, since the plan rests on it. It takes shapes and booleans, no tensors, and launches nothing: its two library calls
(mss_wino_num_tiles, mss_wino_aspp3_supported) are host arithmetic. A new ASPP route adds a field here and a row to
tests/test_aspp_plan_cpu.py."""
import ctypes
import os
from dataclasses import dataclass
from typing import Optional, Tuple

from . import _lib

XT_BUDGET_BYTES = 40 << 30       # all the X' a head forward holds at once (10.6 GB for the three ASPP layers at 2 x 1024 x 2048)


# measured on MI355X (tools/bench_wino.py): F(2x2) 0.87x at 128 channels, 1.24-1.28x at 256, 1.7-2.1x at >= 512;
# F(4x4) 1.29x at 128 channels, 2.0x at 256, 2.4-3.4x at >= 512; F(6x6): 64 -> 128 at 512x1024 1.50 -> 0.8 ms
WINOGRAD_MIN_CHANNELS = {2: 256, 4: 128, 6: 64}


def _on(name):
    return os.environ.get(name, "1") != "0"


def use_winograd(c_in, k_out, stride, in_affine=None, tile=2):
    """Policy: 3x3 stride-1 layers whose channel counts make the two HBM-bound transforms cheaper than the
    MFMA work they remove. MSS_WINOGRAD=0 forces the direct implicit GEMM everywhere."""
    if not _on("MSS_WINOGRAD") or stride != 1:
        return False
    if in_affine is not None and in_affine[0].dim() != 1:
        return False
    lo = WINOGRAD_MIN_CHANNELS[tile]
    return c_in >= lo and k_out >= lo and c_in % 16 == 0 and k_out % 4 == 0


def wino_tile(H, W, dil, max_tile=6):
    """Output-tile edge m of F(m x m, 3x3) for a layer: the one with fewer Winograd-domain elements
    (tiles x (m+2)^2), which decides both the MFMA work and the transform traffic: 1.78 per output pixel for m = 6,
    2.25 for m = 4, 4 for m = 2, unless the dilation sub-grid is so small that the larger tiles are mostly padding
    (e.g. a 12x16 map at dilation 12; the 4x8 sub-grids of dilation 36 at 128x256 stay on 4x4 tiles, the 6x11 ones of
    dilation 24 go from six 4x4 tiles to two 6x6 tiles). m = 6 carries 3x the fp32 rounding error of m = 4 (5.8e-6 vs
    1.9e-6 of the output per layer, tools/wino_matrices.py), so it must save at least 5 % to be chosen, and the caller
    caps it (`max_tile`) on the layers whose error the rest of the network amplifies most (deepv3.wino_cap).
    MSS_WINO_TILE=2|4|6 forces one, MSS_WINO_MAX_TILE=4 keeps the policy off 6x6 tiles everywhere."""
    forced = os.environ.get("MSS_WINO_TILE")
    if forced:
        return int(forced)
    hs, ws = -(-H // dil), -(-W // dil)
    cost = {m: (-(-hs // m)) * (-(-ws // m)) * (m + 2) ** 2 for m in (2, 4, 6)}
    best = 4 if cost[4] < cost[2] else 2
    if min(max_tile, int(os.environ.get("MSS_WINO_MAX_TILE", "6"))) >= 6 and cost[6] <= 0.95 * cost[best]:
        best = 6
    return best


def compose_wanted(hook=False):
    """The switch of the composed route (MSS_ASPP_COMPOSE, default 1): taken under the Winograd policy without a tile hook; the block's
    shapes are the caller's to check (deepv3.DeepWV3Plus._aspp_compose_gate)."""
    return _on("MSS_ASPP_COMPOSE") and not hook and _on("MSS_WINOGRAD")


def tiles(H, W, C, rates, wshapes, hook=False):
    """The tile edges of the three dilated branches where the single-read transforms apply -- rates (d, 2d, 3d), every tile 4 or 6
    under the Winograd policy, no tile hook -- else None. wshapes: the three weights' shapes [K, C, 3, 3]."""
    d = rates[0]
    if hook or tuple(rates) != (d, 2 * d, 3 * d):
        return None
    ts = [wino_tile(H, W, r) for r in rates]
    for ws, t in zip(wshapes, ts):
        if t not in (4, 6) or ws[1] != C or not use_winograd(ws[1], ws[0], 1, None, t):
            return None
    return ts


def pair_tile(N, H, W, ws1, ws2, dil1, dil2, hook=False):
    """Tile edge when two 3x3 / stride-1 layers on the SAME input can share one batched GEMM launch and it pays, else 0: same
    Winograd tile and tile count, K a multiple of 128, and the joint launch fills its rounds of workgroup slots better than each
    alone -- the one-image eval forward: 64 x 1152 x 4096 -> 256 is 1152 narrow tiles = 1.5 rounds of 768 slots (106 TFLOP/s), the
    pair exactly 3 (MSS_WINO_PAIR=0 switches it off)."""
    if not _on("MSS_WINO_PAIR") or hook or tuple(ws1) != tuple(ws2):
        return 0
    k, c = ws1[0], ws1[1]
    t1, t2 = wino_tile(H, W, dil1), wino_tile(H, W, dil2)
    if t1 != t2 or not t1 or not use_winograd(c, k, 1, None, t1) or k % 128:
        return 0
    T1 = _lib.value("mss_wino_num_tiles", N, H, W, dil1, t1)
    if T1 != _lib.value("mss_wino_num_tiles", N, H, W, dil2, t1):
        return 0
    P = (t1 + 2) ** 2

    def eff(positions):                 # the better of the wide (k / 256 column tiles, 512 slots) and narrow (k / 128, 768) launches
        best = 0.0
        for bn, slots in ((256, 512), (128, 768)):
            if k % bn == 0:
                n = positions * -(-T1 // 128) * (k // bn)
                best = max(best, n / (-(-n // slots) * slots))
        return best
    return t1 if eff(2 * P) > eff(P) + 0.1 else 0


def dropped_wanted(route, c0, c1, aff_dims, mask, wshapes):
    """True where the composed route leaves the Dropout2d-zeroed channels of its second factor out of the three dilated branches
    (MSS_ASPP_DROPOUT_COMPACT, default 1): native route, a train-mode mask [N, C1] with its per-sample affine, C0 % 16 == 0,
    48 <= C1 <= 2048, C1 % 16 == 0, (C0 + C1) % 128 == 0, every weight's K a multiple of 128 and at most 4096."""
    if not _on("MSS_ASPP_DROPOUT_COMPACT") or route == "bf16x3" or not mask or tuple(aff_dims) != (1, 2):
        return False
    if c0 % 16 or c1 % 16 or c1 < 48 or c1 > 2048 or (c0 + c1) % 128:
        return False
    return all(ws[0] % 128 == 0 and ws[0] <= 4096 and ws[1] == c0 + c1 for ws in wshapes)


def per_image_products_fit(N, C, Ps, Ts):
    """The 32-bit operand offsets of the per-image (position, image) products and their 65535 batch entries."""
    return not any(4 * p * t * C >= 0xffffffff or t % N or p * N > 65535 for p, t in zip(Ps, Ts))


@dataclass(frozen=True)
class AsppPlan:
    tiles: Optional[Tuple[int, int, int]]  # tile edges of the three dilated branches where the single-read kernels' policy applies
    Ts: Optional[Tuple[int, int, int]]     # their tile counts and
    Ps: Optional[Tuple[int, int, int]]     # Winograd-domain positions (tile + 2)^2; None with tiles
    pair_tile: int            # != 0: the first two branches share one product launch (kernels.conv3x3_pair), on tiles of this edge
    single_read: bool         # one kernel makes the three X' from one read of the map (of its two factors on the composed route)
    dropped: bool             # composed route without the Dropout2d-zeroed channels: kernels.AsppDropped and the per-image products
    dropped_separate: bool    # ... with X' from the materialised compacted map and three plain transforms (MSS_WINO_ASPP3=0)
    gap_from_kernel: bool     # composed route: GAP(w) comes from the two-source kernel (its sums-only mode where it makes no X')
    materialise: bool         # composed route: w = [u ; v] is stored and is the map the branches (and their weight gradients) read
    keep_xt: Tuple[bool, bool, bool]   # per dilated branch: its X' is kept for the weight gradient
    max_bytes: Optional[int]  # what the three X' may take when they are live at once; None: they are kept anyway
    xt_bytes: int             # the three X' under the tile policy, whatever it is: what the budget is held against


def plan(N, H, W, C, wshapes, rates, *, factored=False, c0=0, aff_dims=(1, 1), mask=False, keep=False, wgrad=(False, False, False),
         route="native", hook=False, budget=XT_BUDGET_BYTES):
    """The AsppPlan of one head forward. N, H, W, C: the map ASPP reads (C = C0 + C1 of a kernels.FactoredAct when `factored`, c0 its
    first factor's channels, aff_dims the dimensionality of the two factors' affines, mask: a Dropout2d mask [N, C1] came with it --
    train mode enters only through it); wshapes: the four branch weights' shapes; keep: a backward follows; wgrad: which of
    features[1:]' weights need a gradient; route: kernels.gemm_route(); hook: a tile hook is set; budget: the X' budget in bytes."""
    ws3 = [tuple(s) for s in wshapes[1:]]
    wgrad = tuple(bool(g) for g in wgrad)
    policy = [wino_tile(H, W, r) for r in rates]
    counts = [_lib.value("mss_wino_num_tiles", N, H, W, r, t) for r, t in zip(rates, policy)]
    xt_bytes = sum((t + 2) ** 2 * n for t, n in zip(policy, counts)) * C * 4
    fits = xt_bytes < budget
    # two dilated branches whose Winograd-domain products have the same shape share ONE launch when that fills the chip better
    # (the one-image eval forward: dilations 12 and 24); never when X' is kept for a backward
    pt = 0 if keep else pair_tile(N, H, W, ws3[0], ws3[1], rates[0], rates[1], hook)
    max_bytes = None if (keep and fits) else budget
    keep_xt = tuple(keep and g and fits for g in wgrad)
    ts = tiles(H, W, C, rates, ws3, hook)
    if ts is None:
        # a tile edge of 2, Winograd off, a tile hook: each branch transforms for itself, GAP by its own kernel
        return AsppPlan(None, None, None, pt, False, False, False, False, factored, keep_xt, max_bytes, xt_bytes)
    Ts, Ps = tuple(counts), tuple((t + 2) ** 2 for t in ts)        # (4 or 6 on every rate is the policy's own answer)
    # all three X' are live at once (2.25-4x the map each); a caller that does not keep them for the backward has a budget beyond
    # which each branch transforms for itself again with one X' live at a time
    under = max_bytes is None or 4.0 * sum(p * t for p, t in zip(Ps, Ts)) * C <= max_bytes
    # what the single-read launchers refuse, asked beforehand (host arithmetic: LDS fit, block count, bounds)
    taken = bool(_lib.value("mss_wino_aspp3_supported", N, H, W, C, rates[0], (ctypes.c_int * 3)(*ts), int(factored)))
    aspp3 = _on("MSS_WINO_ASPP3")
    if factored and not pt and under and taken and dropped_wanted(route, c0, C - c0, aff_dims, mask, ws3) \
            and per_image_products_fit(N, C, Ps, Ts):
        return AsppPlan(tuple(ts), Ts, Ps, 0, aspp3, True, not aspp3, True, False, keep_xt, max_bytes, xt_bytes)
    single = aspp3 and under and taken and not (pt and (ts[0] != pt or ts[1] != pt))
    # composed: where X' is not taken from the kernel or is not all kept for the weight gradients, w is materialised and is the
    # map the branches transform for themselves
    mat = factored and (not single or (keep and any(wgrad) and not fits))
    return AsppPlan(tuple(ts), Ts, Ps, pt, single, False, False, factored and taken, mat, keep_xt, max_bytes, xt_bytes)
