"""The packed job plan of the per-image TN weight gradient (csrc/tn_perimg_plan.h) on the GPU: packing alone changes no
bit, the row-split last round changes the tail tiles only and is the ascending sum of its partial tiles, the result stays within the
existing test's bound against float64, and the tail plan is really taken where the mask says so. MSS_WGRAD_TN_SLOTS brings the small
shapes to more than one round. NaN stands behind every buffer, behind the used part of the scratch and in every tile behind an extent."""
import ctypes

import pytest
import torch

import test_gpu_aspp_dropped_kernels as base
from test_tn_perimg_plan_cpu import expected_plan
from multishiftseg_amd import _lib
from multishiftseg_amd._lib import MssConvArgs, call, ptr

pytestmark = pytest.mark.gpu

NAN = float("nan")
TILE = 128 * 128


def _keep_mask(mode, n, C1, g):
    """[n][C1] of {0, 2}. half: p = 0.5 everywhere; all: everything kept; few: fewer than 48 kept (the k_steps floor);
    mixed: image 0 keeps everything, image 1 fewer than 48, a third image half -- three different L."""
    keep = torch.rand((n, C1), device="cuda", generator=g) >= 0.5
    few = torch.zeros(C1, dtype=torch.bool, device="cuda")
    few[torch.randperm(C1, device="cuda", generator=g)[:21]] = True
    if mode == "all":
        keep[:] = True
    elif mode == "few":
        keep[:] = few
    elif mode == "mixed":
        keep[0] = True
        keep[1] = few
    else:
        assert mode == "half"
    keep[:, 5] = keep[:, 5] & (mode == "all")                  # a channel no image keeps (unless every channel is kept)
    return keep.float() * 2.0


def _operands(P, n, Ti, C0, C1, Kout, mode, seed):
    """As the existing file's builder, with the mask chosen: dense X' with exact zeros in the dropped channels, dY', the compacted X'
    with NaN behind every extent."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    C = C0 + C1
    mask = _keep_mask(mode, n, C1, g)
    xt = torch.randn((P, n * Ti, C), device="cuda", generator=g)
    dyt = torch.randn((P, n * Ti, Kout), device="cuda", generator=g)
    drop = base._dropped_state(mask, C0)
    ks, pl = drop.k_steps.cpu().tolist(), drop.place.cpu()
    xc = torch.full((P, n * Ti, C), NAN, device="cuda")
    for i in range(n):
        rows = slice(i * Ti, (i + 1) * Ti)
        xt[:, rows, C0:] *= (mask[i] != 0).float()[None, None, :]
        ext = 16 * ks[i]
        p_i = pl[i, :ext].cuda().long()
        xc[:, rows, :C0] = xt[:, rows, :C0]
        xc[:, rows, C0:C0 + ext] = torch.where((p_i >= 0)[None, None, :], xt[:, rows, C0:][:, :, p_i.clamp_min(0)], torch.zeros((), device="cuda"))
    return mask, drop, xt, xc, dyt, ks


def _tail_tiles(plan, P, n, ktiles, L):
    """(position, image, k tile, c tile) of the plan's tail tiles, in tail-tile order: job numbers full .. live - 1 of the dense
    numbering position, image, k tile, c tile (c tile fastest)."""
    S, _live, full, tail = plan[:4]
    out = []
    for t in range(full, full + tail):
        pos, rem = divmod(t, S)
        for i in range(n):
            if rem < ktiles * L[i]:
                out.append((pos, i, rem // L[i], rem % L[i]))
                break
            rem -= ktiles * L[i]
    assert len(out) == tail
    return out


# (P, n, rows per image, C0, C1, K, mask, MSS_WGRAD_TN_SLOTS or None, tail plan expected)
# The bound of (iii) is 2 x the DENSE kernel's error, and the dense plan cuts the rows of a product with few tiles into ranges to fill
# the chip. A chain's rounding error grows at most in proportion to its length, so the per-image form (one chain of Ti rows per
# image) stays within 2 x the dense form wherever the dense ranges are at least Ti / 2 rows. C = 768 gives that: 432 tiles in two
# ranges of 600 rows at K = 256, 216 tiles in four of 300 at K = 128; so does the existing test's 200-row shape (three ranges of
# 200). At C = 256, K = 128, Ti = 600 the dense product is 72 tiles in five ranges of 240 rows -- 0.4 Ti -- and the whole-tile
# per-image form, the parent's bits, measured 2.09 x it (profiles/aspp_wgrad_packed/tolerances.md): that shape is not a case.
CASES = [
    (36, 2, 600, 128, 640, 256, "half", 128, True),           # L = [4, 4]: 576 live = 4.5 rounds of 128 -> 64 tail tiles halved
    (36, 2, 600, 128, 640, 256, "half", 64, False),           # the same, 9 whole rounds of 64: live % slots == 0, no tail
    (36, 2, 600, 128, 640, 128, "all", 128, True),            # L = ctiles: 432 = 3.375 rounds -> 48 tail tiles halved
    (36, 3, 600, 128, 640, 128, "mixed", 128, True),          # L = [6, 2, 4]: 432 = 3.375 rounds of 128 -> 48 tail tiles halved
    (36, 2, 600, 128, 640, 256, "few", 128, True),            # fewer than 48 kept, L = [2, 2]: 288 = 2.25 rounds -> 32 tail tiles in 3 ranges
    (36, 2, 600, 128, 640, 256, "mixed", 128, True),          # L = [6, 2]: a group ends inside a workgroup
    (36, 3, 200, 128, 128, 256, "half", 64, False),           # 200 rows are a single 256-row range: packed, never split
    (36, 2, 600, 128, 640, 256, "half", None, False),         # the default 1024 slots: below one round
]


@pytest.mark.parametrize("P,n,Ti,C0,C1,Kout,mode,slots,want_tail", CASES)
def test_packed_plan_and_row_split_tail(P, n, Ti, C0, C1, Kout, mode, slots, want_tail, monkeypatch):
    C, T = C0 + C1, n * Ti
    ktiles, ctiles = Kout // 128, C // 128
    mask, drop, xt, xc, dyt, ks = _operands(P, n, Ti, C0, C1, Kout, mode, 17 * P + n + Kout + len(mode) + Ti)
    ref = torch.bmm(dyt.double().cpu().transpose(1, 2), xt.double().cpu())                 # [P][K][C]
    if slots is not None:
        monkeypatch.setenv("MSS_WGRAD_TN_SLOTS", str(slots))
    eff_slots = slots or 1024
    L = [min(ctiles, -(-(C0 + 16 * k) // 128)) for k in ks]
    plan = expected_plan(P, n, ktiles, ctiles, C0 // 16, eff_slots, Ti, 1, ks)
    assert (plan[3] > 0) == want_tail, (L, plan)               # the case is what its comment says
    if mode == "mixed":
        assert len(set(L)) == n
    if mode == "few":
        assert all(k == 3 for k in ks)

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
    ws0 = torch.empty(max(nbytes, 4) // 4, device="cuda")
    du0 = base._with_canary(P * Kout * C)
    call("mss_conv2d_wgrad_f32", ctypes.byref(a0), ptr(dyt), Kout, ptr(du0), C, ptr(ws0), nbytes)
    e0 = base._rel_l2(du0[:P * Kout * C].view(P, Kout, C), ref)

    a1 = args(xc, P * n, Ti)
    a1.k_steps, a1.k_base, a1.k_imgs = ptr(drop.k_steps), C0 // 16, n
    assert _lib.value("mss_conv2d_wgrad_workspace_bytes", ctypes.byref(a1), C) == 0
    size = P * n * Kout * C

    def run(ws, ws_bytes):
        du = base._with_canary(size)
        call("mss_conv2d_wgrad_f32", ctypes.byref(a1), ptr(dyt), Kout, ptr(du), C, ptr(ws), ws_bytes)
        assert torch.isnan(du[size:]).all()
        return du

    # (i) packing alone changes no bit: the unpacked plan and the packed one, both without scratch
    monkeypatch.setenv("MSS_WGRAD_PERIMG_PACK", "0")
    du_unpacked = run(None, 0)
    monkeypatch.setenv("MSS_WGRAD_PERIMG_PACK", "1")
    du_packed = run(None, 0)
    assert torch.equal(base._bits(du_packed), base._bits(du_unpacked))
    dun = du_packed[:size].view(P, n, Kout, C)
    for i in range(n):
        ext = C0 + 16 * ks[i]
        done = L[i] * 128
        assert not torch.isnan(dun[:, i, :, :done]).any()
        assert float(dun[:, i, :, ext:done].abs().max() if done > ext else 0.0) == 0.0
        assert torch.isnan(dun[:, i, :, done:]).all()

    # (ii) with the scratch: NaN in it and behind the part the plan may use
    used = eff_slots * TILE
    ws = base._with_canary(used)
    du_tail = run(ws, used * 4)
    assert torch.isnan(ws[used:]).all()
    tiles = _tail_tiles(plan, P, n, ktiles, L)
    splits = plan[4]
    parts = ws[:used].view(eff_slots, 128, 128)
    written = plan[3] * splits if plan[3] else 0
    # (iv) the tail plan is taken exactly as the mask says: its partial tiles are there, nothing behind them was touched
    assert not torch.isnan(parts[:written]).any()
    assert torch.isnan(parts[written:]).all()
    dut = du_tail[:size].view(P, n, Kout, C)
    same = base._bits(du_tail[:size]).view(P, n, Kout, C) == base._bits(du_packed[:size]).view(P, n, Kout, C)
    changed = 0
    for ti, (pos, i, kt, ct) in enumerate(tiles):
        tile = dut[pos, i, kt * 128:(kt + 1) * 128, ct * 128:(ct + 1) * 128]
        acc = parts[ti].clone()
        for sp in range(1, splits):                            # ascending split order, as the reduce kernel adds them
            acc += parts[sp * plan[3] + ti]
        assert torch.equal(base._bits(tile), base._bits(acc)), (pos, i, kt, ct)
        changed += int(not bool(same[pos, i, kt * 128:(kt + 1) * 128, ct * 128:(ct + 1) * 128].all()))
        same[pos, i, kt * 128:(kt + 1) * 128, ct * 128:(ct + 1) * 128] = True
    assert bool(same.all())                                    # every non-tail tile (and every unwritten one) bit-equal to (i)
    if want_tail:
        assert changed > len(tiles) // 2, (changed, len(tiles))   # another summation order: most tail tiles differ in some bit

    # (iii) gathered and summed over the images, against float64: the existing test's bound, for the packed and the split form
    ratios = []
    for du in (du_packed, du_tail):
        got = torch.empty((P, Kout, C), device="cuda")
        src = du[:size].view(P, n, Kout, C).permute(1, 2, 3, 0).contiguous()
        call("mss_conv2d_pack_weights_f32", ptr(src), ptr(got), Kout, C, P, 1, Kout, C, 0, ptr(drop.col), n, C0)
        nobody = (mask == 0).all(dim=0)
        if bool(nobody.any()):
            assert float(got[:, :, C0:][:, :, nobody].abs().max()) == 0.0
        ratios.append(base._rel_l2(got, ref) / e0)
    print(f"aspp packed wgrad P={P} n={n} rows/img={Ti} C={C0}+{C1} K={Kout} mask={mode} slots={eff_slots} L={L} "
          f"tail={plan[3]}x{splits}: rel-L2 dense {e0:.3e}, packed / dense {ratios[0]:.3f}, packed+tail / dense {ratios[1]:.3f}")
    assert max(ratios) <= 2.0, (ratios, e0)


def test_switches_restore_the_other_plans(monkeypatch):
    """MSS_WGRAD_TN_TAIL=0 keeps whole tiles even with scratch (the scratch stays untouched); a scratch smaller than slots x 64 KiB
    does the same."""
    P, n, Ti, C0, C1, Kout = 36, 2, 600, 128, 128, 128
    C = C0 + C1
    _mask, drop, _xt, xc, dyt, ks = _operands(P, n, Ti, C0, C1, Kout, "few", 3)
    monkeypatch.setenv("MSS_WGRAD_TN_SLOTS", "64")
    assert expected_plan(P, n, 1, 2, C0 // 16, 64, Ti, 1, ks)[3] == 16
    a = MssConvArgs()
    a.x = ptr(xc)
    a.N, a.H, a.W, a.C, a.ldx = 1, 1, Ti, C, C
    a.OH, a.OW, a.K, a.Kpad = 1, Ti, Kout, Kout
    a.R, a.S, a.stride, a.dil, a.pad = 1, 1, 1, 1, 0
    a.batch, a.x_bs, a.y_bs = P * n, Ti * C, Ti * Kout
    a.k_steps, a.k_base, a.k_imgs = ptr(drop.k_steps), C0 // 16, n
    size = P * n * Kout * C
    outs = []
    for tail_env, floats in ((None, 0), ("0", 64 * TILE), (None, 64 * TILE - 4)):
        if tail_env is not None:
            monkeypatch.setenv("MSS_WGRAD_TN_TAIL", tail_env)
        ws = base._with_canary(floats)
        du = base._with_canary(size)
        call("mss_conv2d_wgrad_f32", ctypes.byref(a), ptr(dyt), Kout, ptr(du), C, ptr(ws) if floats else None, floats * 4)
        assert torch.isnan(ws).all() and torch.isnan(du[size:]).all()
        outs.append(du)
        if tail_env is not None:
            monkeypatch.delenv("MSS_WGRAD_TN_TAIL")
    assert torch.equal(base._bits(outs[1]), base._bits(outs[0])) and torch.equal(base._bits(outs[2]), base._bits(outs[0]))
