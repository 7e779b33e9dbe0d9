"""Each OOD-metric kernel of csrc/metric.hip alone, through its C entry point, against tests/ref_ood_metric.py (numpy and Python
integers; pinned to oracle/metric.py by tests/test_ood_metric_ref_cpu.py):

  compaction (single and batch kernel)  per lane: the packed counters, the multiset of inlier keys at the front of the segment and
                                        of OOD keys at its back, every other slot untouched (a sentinel), at every chunk / lane
                                        edge, with a second grid-stride trip, and with scores at the edges of float32;
  gather                                lane order, slot order inside a lane, guards in front and behind;
  rank + finalize                       every multiset of 1..4 OOD and 1..4 inlier scores from three values at 14 recall levels
                                        (the low levels pick recall 0 where inliers lie above every OOD score), and one case on
                                        either side whose rank grid strides twice;
  sort                                  every input misalignment 0..3 crossed with sizes around the 16-byte loads and the tile.

Bounds (none is fitted to what the kernels give): sum(u2_part) is an integer and must be exact; AUROC = u2 / (2 P N) and
FPR = fps / N are one correctly rounded float64 division of exact integers each: one float64 spacing; AP is a sum of P terms
(each a correctly rounded quotient) in some order and a division by P: (P + 2) 2^-52 AP, the a-priori bound of such a sum in
any order -- a dropped or doubled term moves AP by about 1 / P. The worst observed deviations are appended to
ood_metric_kernels.json in the report directory (test_reports/ in the tree, or what MSS_REPORT_DIR names)."""
import ctypes
import itertools
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import ref_ood_metric as R
from conftest import ROOT
from oracle import metric as ometric

pytestmark = pytest.mark.gpu

LEVELS = (0.0, 1e-9, 0.1, 0.125, 0.25, 0.3, 0.375, 0.5, 0.625, 0.7, 0.75, 0.875, 0.95, 1.0)
SENTINEL = 0x5A5A5A5A              # the key of -2.9e-16: no score of these tests
GUARD = 32


def _write_report(report):
    out = os.environ.get("MSS_REPORT_DIR") or os.path.join(ROOT, "test_reports")
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "ood_metric_kernels.json"), "a") as f:
            f.write(json.dumps(report, sort_keys=True) + "\n")
    except OSError:
        pass


@pytest.fixture(scope="module")
def L():
    from multishiftseg_amd import _lib
    return _lib


def at(t, elements=0):
    return ctypes.c_void_p(t.data_ptr() + elements * t.element_size())


def u32(t):
    """int32 device tensor -> uint32 numpy"""
    return t.cpu().numpy().view(np.uint32)


def as_i32(keys):
    """uint32 numpy keys -> int32 device tensor of the same bits"""
    return torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint32).view(np.int32)).cuda()


def sentinel_buffer(n):
    return torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")


def make_map(n, id_in, id_out, seed):
    """Labels: id_in, id_out, 255, a negative value, other ids; from four chunks on, chunk 1 holds no OOD pixel, chunk 2 no inlier,
    chunk 3 neither. Scores: a grid of eighths (ties) with the edge values of float32 scattered over it."""
    rng = np.random.default_rng(seed)
    label = rng.choice([id_in, id_out, 255, -3, id_out + 2, 100], p=[0.45, 0.25, 0.1, 0.05, 0.1, 0.05], size=n).astype(np.int64)
    if n == 1:
        label[0] = id_out
    if n >= 4 * R.CHUNK:
        c = label[R.CHUNK:2 * R.CHUNK]
        c[c == id_out] = id_in
        c = label[2 * R.CHUNK:3 * R.CHUNK]
        c[c == id_in] = id_out
        c = label[3 * R.CHUNK:4 * R.CHUNK]
        c[(c == id_in) | (c == id_out)] = 255
    score = (np.round(rng.standard_normal(n) * 8) / 8).astype(np.float32)
    sp = R.special_scores()
    where = rng.choice(n, size=min(n, 3 * sp.size), replace=False)
    score[where] = np.tile(sp, 3)[:where.size]
    return score, label


def check_lanes(keys, counts, score, label, id_in, id_out, what):
    """keys: the map's 8 cap slots (uint32 numpy), counts: its 8 packed counters (Python integers)"""
    neg, pos, counters, cap = R.lane_layout(score, label, id_in, id_out)
    assert keys.size == R.LANES * cap
    assert counts == counters, what
    for ln in range(R.LANES):
        seg = keys[ln * cap:(ln + 1) * cap]
        a, b = neg[ln].size, pos[ln].size
        assert np.array_equal(np.sort(seg[:a]), neg[ln]), (what, ln, "inlier keys")
        assert np.array_equal(np.sort(seg[cap - b:]), pos[ln]), (what, ln, "OOD keys")
        assert np.all(seg[a:cap - b] == SENTINEL), (what, ln, "slots between the regions")


def counters_of(t):
    return [v & 0xFFFFFFFFFFFFFFFF for v in t.cpu().tolist()]


# ---- compaction -------------------------------------------------------------------------------------------------------------------
COMPACT_N = (1, 63, 64, 65, 4095, 4096, 4097, 8 * 4096, 8 * 4096 + 1, 9 * 4096 + 5)


@pytest.mark.parametrize("ids", [(0, 1), (2, 3)])
@pytest.mark.parametrize("n", COMPACT_N)
def test_compact_lanes(L, n, ids):
    id_in, id_out = ids
    score, label = make_map(n, id_in, id_out, n + id_in)
    cap = L.value("mss_oodm_compact_lanes_cap", n)
    assert cap == R.lanes_cap(n) == -(-(-(-n // 4096)) // 8) * 4096                   # C, reference, OODMeter's formula
    keys = sentinel_buffer(R.LANES * cap + GUARD)
    counts = torch.zeros(R.LANES + 1, dtype=torch.int64, device="cuda")
    counts[R.LANES] = -1
    s, l = torch.from_numpy(score).cuda(), torch.from_numpy(label).cuda()
    L.call("mss_oodm_compact_lanes_f32", at(s), at(l), n, id_in, id_out, at(keys), at(counts))
    host = u32(keys)
    got = counters_of(counts)
    assert got[R.LANES] == 0xFFFFFFFFFFFFFFFF and np.all(host[R.LANES * cap:] == SENTINEL)
    check_lanes(host[:R.LANES * cap], got[:R.LANES], score, label, id_in, id_out, n)


def device_keys(score):
    """score_key in integer arithmetic on the device: int64 tensor of the uint32 keys"""
    u = score.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = torch.where(u == 0x80000000, torch.zeros_like(u), u)
    return torch.where(u >= 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)


def test_compact_lanes_second_grid_trip(L):
    """4096 workgroups of 4096 pixels and 3 chunks + 5 pixels more: workgroups 0..3 take a second chunk, whose lanes are 0..3.
    The expected lanes are built on the device (the same integer rule as ref_ood_metric.score_key / lane_layout)."""
    n = 4096 * 4096 + 3 * 4096 + 5
    id_in, id_out = 0, 1
    g = torch.Generator(device="cuda").manual_seed(3)
    table = torch.tensor([id_in, id_in, id_out, 255, -3, 7], device="cuda")
    label = table[torch.randint(0, 6, (n,), device="cuda", generator=g)]
    score = torch.round(torch.randn(n, device="cuda", generator=g) * 64) / 64
    sp = torch.from_numpy(np.tile(R.special_scores(), 64)).cuda()
    where = torch.randint(0, n, (sp.numel(),), device="cuda", generator=g)
    where[:14] = torch.arange(n - 14, n, device="cuda")                                  # some in the second trip's last chunk
    score[where] = sp
    cap = L.value("mss_oodm_compact_lanes_cap", n)
    assert cap == R.lanes_cap(n) == -(-(-(-n // 4096)) // 8) * 4096
    keys = sentinel_buffer(R.LANES * cap + GUARD)
    counts = torch.zeros(R.LANES, dtype=torch.int64, device="cuda")
    L.call("mss_oodm_compact_lanes_f32", at(score), at(label), n, id_in, id_out, at(keys), at(counts))
    want = device_keys(score)
    lane = (torch.arange(n, device="cuda") // R.CHUNK) % R.LANES
    got = keys[:R.LANES * cap].view(R.LANES, cap).to(torch.int64) & 0xFFFFFFFF
    assert bool((keys[R.LANES * cap:] == SENTINEL).all())
    for ln, c in enumerate(counters_of(counts)):
        a, b = c & 0xFFFFFFFF, c >> 32
        here = lane == ln
        neg, pos = want[here & (label == id_in)], want[here & (label == id_out)]
        assert (a, b) == (neg.numel(), pos.numel()), ln
        assert torch.equal(got[ln, :a].sort()[0], neg.sort()[0]), (ln, "inlier keys")
        assert torch.equal(got[ln, cap - b:].sort()[0], pos.sort()[0]), (ln, "OOD keys")
        assert bool((got[ln, a:cap - b] == SENTINEL).all()), (ln, "slots between the regions")


BATCH_N = (1, 63, 4095, 4096, 4097, 0, 8 * 4096, 8 * 4096 + 1, 9 * 4096 + 5, 64, 65, 5000, 3 * 4096, 20000, 7 * 4096 + 9, 12289)


@pytest.mark.parametrize("sizes,ids", [(BATCH_N, (0, 1)), ((4097, 9 * 4096 + 5), (2, 3))])
def test_compact_lanes_batch(L, sizes, ids):
    """Ragged maps in one launch, one of 0 pixels and one without OOD pixels; the key segments lie GUARD slots apart in one buffer, so
    the segment size the kernel computes per map must be the C function's and OODMeter's."""
    id_in, id_out = ids
    maps = []
    for m, n in enumerate(sizes):
        score, label = make_map(n, id_in, id_out, 100 + m)
        if n == 20000:
            label[label == id_out] = 255
        maps.append((score, label))
    caps = [-(-(-(-n // 4096)) // 8) * 4096 for n in sizes]                            # OODMeter._flush's formula
    for n, cap in zip(sizes, caps):
        assert cap == L.value("mss_oodm_compact_lanes_cap", n) == R.lanes_cap(n)
    first = [0]
    for cap in caps:
        first.append(first[-1] + R.LANES * cap + GUARD)
    keys = sentinel_buffer(first[-1] + GUARD)
    counts = torch.zeros((len(sizes) + 1, R.LANES), dtype=torch.int64, device="cuda")
    counts[len(sizes)] = -1
    dev = [(torch.from_numpy(s if s.size else np.zeros(1, np.float32)).cuda(), torch.from_numpy(l if l.size else np.zeros(1, np.int64)).cuda())
           for s, l in maps]
    b = L.MssOodmBatch()
    for m, (s, l) in enumerate(dev):
        b.score[m], b.label[m], b.n[m] = s.data_ptr(), l.data_ptr(), sizes[m]
        b.keys[m], b.lane_counts[m] = keys.data_ptr() + 4 * first[m], counts.data_ptr() + 8 * R.LANES * m
    L.call("mss_oodm_compact_lanes_batch_f32", ctypes.byref(b), len(sizes), id_in, id_out)
    host = u32(keys)
    got = counters_of(counts.reshape(-1))
    assert got[len(sizes) * R.LANES:] == [0xFFFFFFFFFFFFFFFF] * R.LANES
    for m, (score, label) in enumerate(maps):
        seg = host[first[m]:first[m] + R.LANES * caps[m]]
        check_lanes(seg, got[m * R.LANES:(m + 1) * R.LANES], score, label, id_in, id_out, (m, sizes[m]))
        assert np.all(host[first[m] + R.LANES * caps[m]:first[m + 1]] == SENTINEL), (m, "guard behind the map's segments")
    assert np.all(host[first[-1]:] == SENTINEL)


# ---- gather ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [4096, 2 * 4096])
def test_gather_lanes(L, cap):
    """Hand-built segments of distinct keys: lanes 0 and 5 empty, lane 2 only OOD keys, lane 3 inliers only (the whole segment at
    cap 4096), lane 4 full to the last slot."""
    rng = np.random.default_rng(cap)
    a = [0, 5, 0, 4096, 17, 0, 300, 1]
    b = [0, 0, 9, 0, cap - 17, 0, 700, 0]
    seg = rng.permutation(R.LANES * cap).astype(np.uint32) + np.uint32(0x80000000)       # every slot its own key
    keys = as_i32(seg)
    counts = torch.tensor([x | (y << 32) for x, y in zip(a, b)], dtype=torch.int64, device="cuda")
    neg_out, pos_out = sentinel_buffer(sum(a) + 2 * GUARD), sentinel_buffer(sum(b) + 2 * GUARD)
    L.call("mss_oodm_gather_lanes_u32", at(keys), cap, at(counts), at(neg_out, GUARD), at(pos_out, GUARD))
    want_neg = np.concatenate([seg[ln * cap:ln * cap + a[ln]] for ln in range(R.LANES)])
    want_pos = np.concatenate([seg[(ln + 1) * cap - b[ln]:(ln + 1) * cap] for ln in range(R.LANES)])
    for got, want in ((u32(neg_out), want_neg), (u32(pos_out), want_pos)):
        assert np.all(got[:GUARD] == SENTINEL) and np.all(got[GUARD + want.size:] == SENTINEL)
        assert np.array_equal(got[GUARD:GUARD + want.size], want)


# ---- rank and finalize -----------------------------------------------------------------------------------------------------------
def spacings(got, want):
    """|got - want| in float64 spacings of want (want: the correctly rounded quotient)"""
    return abs(got - want) / float(np.spacing(want)) if got != want else 0.0


def check_measures(out, P, N, u2, ap, fps, worst, what):
    """out: the kernel's three float64 against the exact (u2, ap, fps); returns the violated checks."""
    bad = []
    d = spacings(out[0], float(Fraction(u2, 2 * P * N)))
    worst["auroc_spacings"] = max(worst.get("auroc_spacings", 0.0), d)
    if not d <= 1:
        bad.append((what, "auroc", out[0], u2 / (2 * P * N)))
    d = spacings(out[2], float(Fraction(fps, N)))
    worst["fpr_spacings"] = max(worst.get("fpr_spacings", 0.0), d)
    if not (d <= 1 and round(out[2] * N) == fps):
        bad.append((what, "fpr", out[2], fps / N))
    if math.isfinite(out[1]):
        ratio = float(abs(Fraction(out[1]) - ap) / (Fraction(P + 2, 2 ** 52) * ap))
    else:
        ratio = math.inf
    worst["ap_ratio_to_bound"] = max(worst.get("ap_ratio_to_bound", 0.0), ratio)
    if not ratio <= 1:
        bad.append((what, "ap", out[1], float(ap)))
    return bad


def test_measures_three_value_enumeration(L):
    """16,184 cases queued on one stream into one buffer, one copy back. A kernel that cannot pick recall 0 misses 998 of them,
    all at levels <= 0.375."""
    sets = [c for k in range(1, 5) for c in itertools.combinations_with_replacement((0.0, 1.0, 2.0), k)]
    pairs = [(p, q) for p in sets for q in sets]
    cases = len(pairs) * len(LEVELS)
    assert cases == 16184
    packed, where, used = [], [], 0
    for p, q in pairs:
        pk, nk = np.sort(R.score_key(np.float32(p))), np.sort(R.score_key(np.float32(q)))
        where.append((used, used + pk.size))
        packed += [pk, nk]
        used += pk.size + nk.size
    keys = as_i32(np.concatenate(packed))
    assert L.value("mss_oodm_rank_blocks", 4) == 1
    # one buffer: [cases + 1][3] results, then one u2 and one ap partial per pair (+ a guard each); -1 is a NaN as a float64
    blob = torch.full((3 * (cases + 1) + 2 * (len(pairs) + 1),), -1, dtype=torch.int64, device="cuda")
    o_u2, o_ap = 3 * (cases + 1), 3 * (cases + 1) + len(pairs) + 1
    for i, ((p, q), (po, no)) in enumerate(zip(pairs, where)):
        for k, level in enumerate(LEVELS):
            L.call("mss_oodm_measures_f64", at(keys, po), len(p), at(keys, no), len(q), ctypes.c_double(level),
                   at(blob, o_u2 + i), at(blob, o_ap + i), at(blob, 3 * (i * len(LEVELS) + k)))
    host = blob.cpu().numpy()
    out = host[:o_u2].view(np.float64).reshape(cases + 1, 3)
    u2_part, ap_part = host[o_u2:o_ap], host[o_ap:].view(np.float64)
    assert np.all(host[3 * cases:o_u2] == -1) and u2_part[-1] == -1 and host[-1] == -1   # the three guards
    bad, worst, fpr_misses = [], {}, 0
    for i, (p, q) in enumerate(pairs):
        u2, ap, fps = R.measures_levels(packed[2 * i], packed[2 * i + 1], LEVELS)
        if int(u2_part[i]) != u2:
            bad.append(((p, q), "u2_part", int(u2_part[i]), u2))
        if not abs(Fraction(float(ap_part[i])) - ap * len(p)) <= Fraction(len(p) + 2, 2 ** 52) * ap * len(p):
            bad.append(((p, q), "ap_part", float(ap_part[i]), float(ap * len(p))))
        for k, level in enumerate(LEVELS):
            row = out[i * len(LEVELS) + k].tolist()
            miss = check_measures(row, len(p), len(q), u2, ap, fps[k], worst, (p, q, level))
            fpr_misses += any(m[1] == "fpr" for m in miss)
            bad += miss
    print(f"three-value enumeration: {cases} cases, {fpr_misses} with a wrong FPR, worst {worst}")
    _write_report({"check": "measures_three_value_enumeration", "cases": cases, "fpr_mismatches": fpr_misses,
                   "bounds": {"auroc_spacings": 1, "fpr_spacings": 1, "ap_ratio_to_bound": 1}, "worst": worst})
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("side", ["many_ood", "many_inliers"])
def test_measures_rank_grid_strides_twice(L, side):
    """P = 4096 x 256 + 300 OOD keys on 300 distinct scores against 777 inliers: the first 300 threads of the rank grid take a
    second key. And the mirror: 5 OOD keys against as many inliers (binary searches over 2^20 keys, one block)."""
    rng = np.random.default_rng(17)
    big, small = 4096 * 256 + 300, 777 if side == "many_ood" else 5
    many = (rng.integers(0, 300, big) / 4).astype(np.float32)
    few = (rng.integers(-20, 320, small) / 4).astype(np.float32)                          # some below and some above every one of `many`
    few[:2] = [80.0, -1.0]
    pos, neg = (many, few) if side == "many_ood" else (few, many)
    pk, nk = np.sort(R.score_key(pos)), np.sort(R.score_key(neg))
    P, N = pk.size, nk.size
    nb = L.value("mss_oodm_rank_blocks", P)
    assert nb == (4096 if side == "many_ood" else 1)
    dp, dn = as_i32(pk), as_i32(nk)
    u2_part = torch.full((nb + GUARD,), -1, dtype=torch.int64, device="cuda")
    ap_part = torch.full((nb + GUARD,), math.nan, dtype=torch.float64, device="cuda")
    out = torch.full((len(LEVELS) + 1, 3), math.nan, dtype=torch.float64, device="cuda")
    for k, level in enumerate(LEVELS):
        L.call("mss_oodm_measures_f64", at(dp), P, at(dn), N, ctypes.c_double(level), at(u2_part), at(ap_part), at(out, 3 * k))
    u2_host, ap_host, out = u2_part.cpu().tolist(), ap_part.cpu().numpy(), out.cpu().numpy()
    assert all(v >= 0 for v in u2_host[:nb]) and u2_host[nb:] == [-1] * GUARD          # exactly nb entries written
    assert np.all(np.isfinite(ap_host[:nb])) and np.all(np.isnan(ap_host[nb:])) and np.all(np.isnan(out[-1]))
    u2, ap, fps = R.measures_levels(pk, nk, LEVELS)
    assert sum(u2_host[:nb]) == u2
    bad, worst = [], {}
    for k, level in enumerate(LEVELS):
        bad += check_measures(out[k].tolist(), P, N, u2, ap, fps[k], worst, (side, level))
    print(f"{side}: P {P} N {N}, worst {worst}")
    _write_report({"check": "measures_" + side, "P": P, "N": N, "bounds": {"auroc_spacings": 1, "fpr_spacings": 1, "ap_ratio_to_bound": 1},
                   "worst": worst, "u2_sum_exact": True})
    assert not bad, bad


# ---- the public class ------------------------------------------------------------------------------------------------------------
def against_oracle(got, score, label, level=0.95, id_in=0, id_out=1):
    """FPR with ==; AUROC and AP within n 2^-52: the oracle sums at most n float64 terms <= 1 (the kernels' own error is far below,
    see the kernel checks above)."""
    want = ometric.eval_ood_measure(score.reshape(-1), label.reshape(-1), id_in, id_out, recall_level=level)
    assert got is not None and want is not None
    tol = score.size * 2.0 ** -52
    dev = max(abs(got[0] - want[0]), abs(got[1] - want[1]))
    print(f"level {level}: max |auroc, ap - oracle| {dev:.3e}, bound {tol:.3e}; fpr {got[2]!r} against {want[2]!r}")
    assert dev <= tol, (got, want)
    assert got[2] == want[2], (level, got, want)
    return dev / tol


@pytest.mark.parametrize("level", [0.0, 0.05, 0.5, 0.95, 1.0])
def test_meter_recall_level(level):
    from multishiftseg_amd import metric as M
    rng = np.random.default_rng(23)
    label = rng.choice([0, 1, 255], p=[0.7, 0.2, 0.1], size=(40, 50)).astype(np.int64)
    score = (np.round((rng.standard_normal((40, 50)) + 0.8 * (label == 1)) * 4) / 4).astype(np.float32)
    top = np.argwhere(label == 0)[:7]
    score[top[:, 0], top[:, 1]] = 50.0 + np.arange(7, dtype=np.float32) // 2              # the top scores are inliers
    few_l = np.zeros(50, dtype=np.int64)
    few_l[[3, 20, 41]] = 1                                                                 # P = 3
    few_s = rng.standard_normal(50).astype(np.float32)
    few_s[[3, 20, 41]] = [0.5, 0.5, 1.5]
    worst = 0.0
    for s, l in ((score, label), (few_s, few_l)):
        m = M.OODMeter(recall_level=level)
        m.update(torch.from_numpy(s).cuda(), torch.from_numpy(l).cuda())
        worst = max(worst, against_oracle(m.compute(), s, l, level))
    _write_report({"check": f"meter_recall_level_{level}", "bounds": {"auroc_ap_ratio_to_bound": 1, "fpr": "=="},
                   "worst": {"auroc_ap_ratio_to_bound": worst, "fpr": "=="}})


@pytest.mark.parametrize("kind", ["fp16", "transposed", "requires_grad", "uint8_label", "int32_label"])
def test_meter_converts_inputs(kind):
    """What OODMeter's _flat converts before the kernel sees it, against the oracle on the converted arrays."""
    from multishiftseg_amd import metric as M
    g = torch.Generator(device="cuda").manual_seed(29)
    label = torch.tensor([0, 0, 1, 255, 0, 1], device="cuda")[torch.randint(0, 6, (40, 50), device="cuda", generator=g)]
    score = torch.round((torch.randn(40, 50, device="cuda", generator=g) + 0.8 * (label == 1)) * 8) / 8
    if kind == "fp16":
        score = (score + 1e-3).half()
    elif kind == "transposed":
        score = score.t().contiguous().t()                                                  # [40, 50] with strides (1, 40)
        assert not score.is_contiguous()
    elif kind == "requires_grad":
        score = score.requires_grad_(True)
    elif kind == "uint8_label":
        label = label.to(torch.uint8)
    else:
        label = torch.where(label == 255, torch.full_like(label, -3), label).to(torch.int32)
    got = M.eval_ood_measure(score, label)
    worst = against_oracle(got, score.detach().float().contiguous().cpu().numpy(), label.long().contiguous().cpu().numpy())
    _write_report({"check": "meter_converts_" + kind, "bounds": {"auroc_ap_ratio_to_bound": 1, "fpr": "=="},
                   "worst": {"auroc_ap_ratio_to_bound": worst, "fpr": "=="}})


# ---- sort ------------------------------------------------------------------------------------------------------------------------
SORT_N = (1, 2, 3, 4, 5, 7, 8, 9, 4093, 4094, 4095, 4096, 4097, 4098, 4099, 2 * 4096 - 1, 2 * 4096, 2 * 4096 + 1)


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_sort_every_misalignment(L, monkeypatch, offset):
    """The histogram kernel reads 16 bytes at a time from the first aligned key on and the 0..3 keys before it one by one: every
    input misalignment against every size around those loads and around the tile, on both sort routes; guards around keys_out."""
    g = torch.Generator(device="cuda").manual_seed(offset)
    for n in SORT_N:
        keys = torch.randint(-2 ** 31, 2 ** 31, (n,), device="cuda", generator=g, dtype=torch.int64)
        if n > 8:
            keys[::3] = keys[0]                                                             # ties
        pad = sentinel_buffer(n + 8)
        assert pad.data_ptr() % 16 == 0
        pad[offset:offset + n] = keys.to(torch.int32)
        want = torch.sort(keys & 0xFFFFFFFF)[0]
        temp = torch.empty(L.value("mss_oodm_sort_temp_bytes", n), dtype=torch.uint8, device="cuda")
        for route in ("own", "rocprim"):
            monkeypatch.setenv("MSS_OODM_SORT", route)
            out = sentinel_buffer(n + 8)
            L.call("mss_oodm_sort_u32", at(pad, offset), at(out, 4), n, at(temp), temp.numel())
            assert torch.equal(out[4:4 + n].to(torch.int64) & 0xFFFFFFFF, want), (route, n)
            assert bool((out[:4] == SENTINEL).all()) and bool((out[4 + n:] == SENTINEL).all()), (route, n)
