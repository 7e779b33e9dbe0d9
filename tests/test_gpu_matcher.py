"""GPU: the Hungarian matcher on HIP (csrc/m2f_match.hip, multishiftseg_amd/matcher.py) against the fixture recorded from the
reference's own HungarianMatcher (tests/golden/m2f_matcher.npz), against scipy where it is installed, and against the float64
restatement of tests/ref_matcher.py on edge shapes.

The cost bound: max|C_hip - C_float64| <= 8 x floor, floor = max|C_float32 - C_float64| of the reference arithmetic itself on the
same inputs (recorded in the fixture; from the restatement run in float32 for the edge shapes). The x8 covers a different but
equally sound fp32 summation order; the reference's own error sits at about 2 ulp of the cost."""
import numpy as np
import pytest
import torch

import poison
import ref_matcher
from conftest import golden
from multishiftseg_amd import HungarianMatcher
from multishiftseg_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _case(tag):
    g = golden("m2f_matcher")
    c = {k[len(tag) + 1:]: g[k] for k in g.files if k.startswith(tag + "_")}
    c["weights"] = tuple(float(v) for v in g["weights"])
    return c


def _dev_case(c):
    S = c["points"].shape[0]
    return dict(masks=[torch.from_numpy(c["pred_masks"][s]).to(DEV) for s in range(S)],
                logits=[torch.from_numpy(c["pred_logits"][s]).to(DEV) for s in range(S)],
                tmask=torch.from_numpy(c["tmasks"]).to(DEV), tstart=torch.from_numpy(c["tstart"]).to(DEV),
                labels=torch.from_numpy(c["labels"]).to(DEV), points=torch.from_numpy(c["points"]).to(DEV))


def _pixel_major(m, ldq):
    """NCHW [B,Q,h,w] -> [B,h,w,ldq]; the padding of the query axis holds NaN: the kernel never reads it."""
    B, Q, h, w = m.shape
    out = torch.full((B, h, w, ldq), float("nan"), device=m.device)
    out[..., :Q] = m.permute(0, 2, 3, 1)
    return out


def _targets(c, dtype=torch.bool):
    ts = c["tstart"]
    return [{"labels": torch.from_numpy(c["labels"][ts[b]:ts[b + 1]].astype(np.int64)).to(DEV),
             "masks": torch.from_numpy(c["tmasks"][ts[b]:ts[b + 1]]).to(DEV).to(dtype)} for b in range(len(ts) - 1)]


def _pairs_of(match_row, T):
    q = match_row[:T]
    order = np.argsort(q)
    return q[order].tolist(), order.tolist()


@pytest.mark.parametrize("tag", ["a", "b"])
def test_cost_against_the_reference_fixture_in_both_layouts(tag):
    c = _case(tag)
    d = _dev_case(c)
    Tmax = c["cost_ref64"].shape[3]
    args = (d["tmask"], d["tstart"], d["labels"], d["points"], c["weights"])
    cost = K.m2f_match_cost(d["masks"], d["logits"], *args, Tmax=Tmax)
    dev = float(np.abs(cost.cpu().numpy().astype(np.float64) - c["cost_ref64"]).max())
    floor = float(c["floor"])
    print(f"case {tag}: max|C_hip - ref64| {dev:.3e}, floor {floor:.3e}, bound {8 * floor:.3e}")
    assert dev <= 8 * floor
    for ldq in (100, 104):
        pm = K.m2f_match_cost([_pixel_major(m, ldq) for m in d["masks"]], d["logits"], *args, Tmax=Tmax, pixel_major=True)
        assert torch.equal(pm, cost), ldq


@pytest.mark.parametrize("tag", ["a", "b"])
def test_fixture_end_to_end_returns_the_reference_indices(tag):
    c = _case(tag)
    d = _dev_case(c)
    S, B = c["points"].shape[:2]
    T = np.diff(c["tstart"])
    m = HungarianMatcher(cost_class=c["weights"][0], cost_mask=c["weights"][1], cost_dice=c["weights"][2], num_points=c["points"].shape[2])
    steps = [{"pred_logits": d["logits"][s], "pred_masks": d["masks"][s]} for s in range(S)]
    want = [[_pairs_of(c["match"][s, b], T[b]) for b in range(B)] for s in range(S)]
    for dtype in (torch.bool, torch.uint8, torch.float32):
        got = m.match_steps(steps, _targets(c, dtype), point_coords=d["points"])
        assert [[(i.tolist(), j.tolist()) for i, j in step] for step in got] == want
    as_dict = dict(steps[0], aux_outputs=steps[1:])
    got = m.match_steps(as_dict, _targets(c), point_coords=d["points"])
    assert [[(i.tolist(), j.tolist()) for i, j in step] for step in got] == want
    for s in range(S):
        got = m(steps[s], _targets(c), point_coords=d["points"][s])
        assert all(i.dtype == torch.int64 and j.dtype == torch.int64 and not i.is_cuda for i, j in got)
        assert [(i.tolist(), j.tolist()) for i, j in got] == want[s]
    table = m.match_steps(steps, _targets(c), point_coords=d["points"], device_only=True)
    assert table.is_cuda and table.dtype == torch.int32 and np.array_equal(table.cpu().numpy(), c["match"])
    assert int(m.last_status.abs().sum()) == 0
    drawn = m.match_steps(steps, _targets(c))                      # its own points: a valid matching of the right sizes
    assert [[len(i) for i, _ in step] for step in drawn] == [[int(t) for t in T]] * S


SHAPES = [(1, 1), (1, 100), (19, 100), (33, 33), (64, 65), (128, 128), (20, 127)]


def _solve(C, T):
    """C [Q,Tmax] numpy float32 -> (q_of_t list, status) from the HIP solver."""
    match, status = K.m2f_match_assign(torch.from_numpy(C)[None, None].to(DEV), [T])
    return match[0, 0, :T].cpu().tolist(), int(status[0, 0])


@pytest.mark.parametrize("T,Q", SHAPES)
def test_assignment_against_scipy(T, Q):
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rng = np.random.default_rng(1000 * T + Q)
    for trial in range(3):
        C = (rng.standard_normal((Q, T)) * 5).astype(np.float32)
        got, status = _solve(C, T)
        ri, rj = lsa(C)
        assert status == 0 and _pairs_of(np.array(got), T) == (ri.tolist(), rj.tolist())
    for trial in range(3):                                         # deliberate ties: totals agree exactly, indices may differ
        C = rng.integers(0, 4, (Q, T)).astype(np.float32)
        got, status = _solve(C, T)
        ri, rj = lsa(C)
        assert status == 0 and len(set(got)) == T and min(got) >= 0 and max(got) < Q
        assert ref_matcher.total(C, got) == float(C[ri, rj].astype(np.float64).sum())
    pad = min(3, 128 - T)                                          # the table holds at most 128 targets
    Cpad = np.zeros((Q, T + pad), np.float32)                      # padded columns hold anything: -1 in the table
    Cpad[:, :T] = (rng.standard_normal((Q, T)) * 5).astype(np.float32)
    Cpad[:, T:] = np.nan
    match, status = K.m2f_match_assign(torch.from_numpy(Cpad)[None, None].to(DEV), [T])
    ri, rj = lsa(Cpad[:, :T])
    assert int(status[0, 0]) == 0 and match[0, 0, T:].cpu().tolist() == [-1] * pad
    assert _pairs_of(match[0, 0].cpu().numpy(), T) == (ri.tolist(), rj.tolist())


def test_invalid_costs_end_with_status_1_and_a_value_error():
    """A NaN, a -inf or a row of +inf is scipy's ValueError: status 1, match -1, the neighbours in the same call solved."""
    rng = np.random.default_rng(3)
    Q, T = 100, 7
    C = (rng.standard_normal((1, 5, Q, T)) * 5).astype(np.float32)
    C[0, 1, 17, 3] = np.nan
    C[0, 2, :, 5] = np.inf                                          # target 5 has no finite query
    C[0, 3, 0, 0] = -np.inf
    C[0, 4, 40, 2] = np.inf                                         # a single +inf entry is allowed
    match, status = K.m2f_match_assign(torch.from_numpy(C).to(DEV), [T] * 5)
    assert status.cpu().tolist() == [[0, 1, 1, 1, 0]]
    match = match.cpu().numpy()
    assert (match[0, 1:4] == -1).all()
    for b in (0, 4):
        assert match[0, b].tolist() == ref_matcher.lsap(C[0, b].T).tolist()
    _, status = K.m2f_match_assign(torch.from_numpy(C[:, :1]).to(DEV), [T + 1])        # a count beyond the table
    assert status.cpu().tolist() == [[1]]

    c = _case("a")
    d = _dev_case(c)
    m = HungarianMatcher(*c["weights"], num_points=c["points"].shape[2])
    masks = d["masks"][0].clone()
    masks[1, 5] = float("nan")
    with pytest.raises(ValueError):
        m({"pred_logits": d["logits"][0], "pred_masks": masks}, _targets(c), point_coords=d["points"][0])
    labels = _targets(c)
    labels[0]["labels"][0] = 20                                     # a label outside the C+1 classes
    with pytest.raises(ValueError):
        m({"pred_logits": d["logits"][0], "pred_masks": d["masks"][0]}, labels, point_coords=d["points"][0])


def _edge_case(rng, S, B, Q, P, hw, T, big_logits=False):
    h, w = hw
    H, W = 9, 4
    C1 = 6
    n = sum(T)
    tmasks = (rng.random((n, H, W)) < 0.5).astype(np.uint8)
    if n >= 2:
        tmasks[0] = 0                                               # an all-zero and an all-one target mask
        tmasks[1] = 1
    labels = rng.integers(0, C1 - 1, n).astype(np.int32)
    tstart = np.concatenate([[0], np.cumsum(T)]).astype(np.int32)
    masks = (rng.standard_normal((S, B, Q, h, w)) * 3).astype(np.float32)
    if big_logits:
        masks = np.where(rng.random(masks.shape) < 0.5, np.float32(80), np.float32(-80)).astype(np.float32)
    logits = (rng.standard_normal((S, B, Q, C1)) * 2).astype(np.float32)
    pts = rng.random((S, B, P, 2), dtype=np.float32)
    below1 = np.nextafter(np.float32(1), np.float32(0))
    special = [(0, 0), (0.5 / W, 0.5 / H), (0.5 / w, 0.5 / h), (below1, below1), (0, below1), (below1, 0.5 / H)]
    for k, xy in enumerate(special[:max(0, P - 1)]):                # border taps and taps outside the map
        pts[:, :, k] = np.array(xy, np.float32)
    return dict(pred_masks=masks, pred_logits=logits, tmasks=tmasks, labels=labels, tstart=tstart, points=pts)


EDGES = {
    "q1_mask1x1": dict(S=10, B=3, Q=1, P=63, hw=(1, 1), T=[1, 0, 1]),
    "p1": dict(S=1, B=1, Q=100, P=1, hw=(1, 7), T=[3]),
    "q33_tb0_between": dict(S=1, B=3, Q=33, P=65, hw=(1, 7), T=[4, 0, 2]),
    "s10_q100": dict(S=10, B=3, Q=100, P=257, hw=(5, 3), T=[3, 0, 5]),
    "q128_t17_pm80": dict(S=1, B=1, Q=128, P=257, hw=(5, 3), T=[17], big_logits=True),
    "p12544": dict(S=1, B=3, Q=100, P=12544, hw=(5, 3), T=[2, 0, 3]),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_edge_shapes_end_to_end_against_the_float64_restatement(name):
    cfg = EDGES[name]
    rng = np.random.default_rng(sorted(EDGES).index(name) + 50)
    c = _edge_case(rng, **cfg)
    w = (2.0, 5.0, 5.0)
    S, B, Q, T = cfg["S"], cfg["B"], cfg["Q"], cfg["T"]
    Tmax = max(T)
    ts = c["tstart"]
    c64, floor = {}, 0.0
    for s in range(S):
        for b in range(B):
            args = (c["pred_logits"][s, b], c["pred_masks"][s, b], c["tmasks"][ts[b]:ts[b + 1]], c["labels"][ts[b]:ts[b + 1]], c["points"][s, b], w)
            c64[s, b] = ref_matcher.cost_matrix(*args).numpy()
            if T[b]:
                floor = max(floor, float(np.abs(ref_matcher.cost_matrix(*args, dtype=torch.float32).numpy().astype(np.float64) - c64[s, b]).max()))
    bound = 8 * floor
    d = _dev_case(c)
    cost, match, status, _ = K.m2f_match_cost(d["masks"], d["logits"], d["tmask"], d["tstart"], d["labels"], d["points"], w, Tmax=Tmax, solve=True)
    again = K.m2f_match_cost(d["masks"], d["logits"], d["tmask"], d["tstart"], d["labels"], d["points"], w, Tmax=Tmax, solve=True)
    assert torch.equal(cost, again[0]) and torch.equal(match, again[1])                   # two runs are bit-identical
    cost, match = cost.cpu().numpy(), match.cpu().numpy()
    assert int(status.abs().sum()) == 0
    dev = max(float(np.abs(cost[s, b, :, :T[b]].astype(np.float64) - c64[s, b]).max()) for s in range(S) for b in range(B) if T[b])
    print(f"{name}: max|C_hip - float64| {dev:.3e}, floor {floor:.3e}, bound {bound:.3e}")
    assert dev <= bound
    for s in range(S):
        for b in range(B):
            assert (cost[s, b, :, T[b]:] == 0).all() and (match[s, b, T[b]:] == -1).all()
            got = match[s, b, :T[b]].tolist()
            assert len(set(got)) == T[b] and all(0 <= q < Q for q in got)
            if T[b]:                                                # optimal under the float64 cost, to the cost's own bound
                best = ref_matcher.total(c64[s, b], ref_matcher.lsap(c64[s, b].T))
                assert ref_matcher.total(c64[s, b], got) <= best + 2 * T[b] * bound
    m = HungarianMatcher(*w, num_points=cfg["P"])
    steps = [{"pred_logits": d["logits"][s], "pred_masks": d["masks"][s]} for s in range(S)]
    pairs = m.match_steps(steps, _targets(c), point_coords=d["points"])
    for s in range(S):
        for b in range(B):
            i, j = pairs[s][b]
            assert (i.tolist(), j.tolist()) == _pairs_of(match[s, b], T[b]) and i.dtype == torch.int64 and len(i) == T[b]


def test_poisoned_scratch_and_padding_change_nothing():
    """Two clean runs and one run under each poison of tests/poison.py are bit-identical: no padding column, workspace element or
    output is read before it is written, and the chunk merge has one order."""
    c = _case("a")
    d = _dev_case(c)
    Tmax = c["cost_ref64"].shape[3]
    counts = torch.from_numpy(np.diff(c["tstart"]).astype(np.int32)).to(DEV)
    cost = K.m2f_match_cost(d["masks"], d["logits"], d["tmask"], d["tstart"], d["labels"], d["points"], c["weights"], Tmax=Tmax)
    m = HungarianMatcher(*c["weights"], num_points=c["points"].shape[2])
    steps = [{"pred_logits": lg, "pred_masks": mk} for lg, mk in zip(d["logits"], d["masks"])]
    targets = _targets(c)

    def run_cost():
        return list(K.m2f_match_cost(d["masks"], d["logits"], d["tmask"], d["tstart"], d["labels"], d["points"], c["weights"], Tmax=Tmax,
                                     solve=True)[:3])
    runs = poison.poison_runs(run_cost, bitwise=True)
    assert np.array_equal(runs["clean"][1].numpy(), c["match"])
    poison.poison_runs(lambda: list(K.m2f_match_assign(cost, counts)), bitwise=True)
    runs = poison.poison_runs(lambda: m.match_steps(steps, targets, point_coords=d["points"]), bitwise=True)
    assert len(runs["clean"]) == 2 * len(steps) * len(targets)
    poison.poison_runs(lambda: m.match_steps(steps, targets, point_coords=d["points"], device_only=True), bitwise=True)
