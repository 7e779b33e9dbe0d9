"""CPU: the host side of the Hungarian matcher (multishiftseg_amd/matcher.py): the reference's interface, the refusals, the
conversion of a device match table into the reference's pairs, the workspace arithmetic, and the test yardstick itself
(tests/ref_matcher.py) against the fixture recorded from the reference (tests/golden/m2f_matcher.npz) and against brute force."""
import numpy as np
import pytest
import torch

import ref_matcher
from conftest import golden
from multishiftseg_amd import HungarianMatcher, _lib
from multishiftseg_amd import kernels as K
from multishiftseg_amd.matcher import pairs_from_table

CASES = ("a", "b")


def test_constructor_repr_and_assertion_mirror_the_reference():
    m = HungarianMatcher(cost_class=2.0, cost_mask=5.0, cost_dice=5.0, num_points=12544)
    assert (m.cost_class, m.cost_mask, m.cost_dice, m.num_points) == (2.0, 5.0, 5.0, 12544)
    assert repr(m) == "Matcher HungarianMatcher\n    cost_class: 2.0\n    cost_mask: 5.0\n    cost_dice: 5.0"
    d = HungarianMatcher()
    assert (d.cost_class, d.cost_mask, d.cost_dice, d.num_points) == (1, 1, 1, 0)
    with pytest.raises(AssertionError, match="all costs cant be 0"):
        HungarianMatcher(0, 0, 0)
    HungarianMatcher(0, 0, 1)


def _problem(B=2, Q=5, T=(2, 1)):
    outputs = {"pred_logits": torch.zeros(B, Q, 4), "pred_masks": torch.zeros(B, Q, 3, 3)}
    targets = [{"labels": torch.zeros(t, dtype=torch.int64), "masks": torch.zeros(t, 6, 6, dtype=torch.bool)} for t in T]
    return outputs, targets


def test_there_is_no_cpu_path():
    outputs, targets = _problem()
    m = HungarianMatcher(num_points=8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(outputs, targets)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.match_steps([outputs, outputs], targets, point_coords=torch.rand(2, 2, 8, 2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.m2f_match_assign(torch.zeros(1, 1, 4, 2), [2])
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.m2f_match_cost(outputs["pred_masks"], outputs["pred_logits"], torch.zeros(3, 6, 6, dtype=torch.uint8),
                         torch.tensor([0, 2, 3], dtype=torch.int32), torch.zeros(3, dtype=torch.int32), torch.rand(1, 2, 8, 2))


def test_more_targets_than_queries_and_more_than_128_queries_are_refused():
    m = HungarianMatcher(num_points=8)
    outputs, targets = _problem(Q=3, T=(2, 4))
    with pytest.raises(NotImplementedError):
        m(outputs, targets)
    outputs, targets = _problem(Q=129, T=(2, 1))
    with pytest.raises(NotImplementedError):
        m(outputs, targets)


def test_match_table_to_sorted_pairs():
    """[S,B,Tmax] table (query of target m, -1 padding) -> per step, per image (index_i ascending, index_j), T_b = 0 included."""
    table = torch.tensor([[[7, 2, 5], [-1, -1, -1], [4, -1, -1]],
                          [[0, 1, 2], [-1, -1, -1], [9, -1, -1]]], dtype=torch.int32)
    out = pairs_from_table(table, [3, 0, 1])
    assert len(out) == 2 and all(len(step) == 3 for step in out)
    i, j = out[0][0]
    assert i.dtype == j.dtype == torch.int64 and i.tolist() == [2, 5, 7] and j.tolist() == [1, 2, 0]
    i, j = out[0][1]
    assert i.dtype == j.dtype == torch.int64 and i.numel() == 0 and j.numel() == 0
    assert [t.tolist() for t in out[0][2]] == [[4], [0]]
    assert [t.tolist() for t in out[1][0]] == [[0, 1, 2], [0, 1, 2]]
    assert [t.tolist() for t in out[1][2]] == [[9], [0]]


@pytest.mark.parametrize("tag", CASES)
def test_ref_matcher_reproduces_the_reference_fixture(tag):
    """The float64 restatement gives the reference's float64 cost to rounding, its float32 run stays at the recorded floor, and
    the numpy solver returns the reference's indices from either."""
    g = golden("m2f_matcher")
    w = tuple(g["weights"])
    ts, floor = g[f"{tag}_tstart"], float(g[f"{tag}_floor"])
    S, B = g[f"{tag}_points"].shape[:2]
    assert floor == float(np.abs(g[f"{tag}_cost_ref32"].astype(np.float64) - g[f"{tag}_cost_ref64"]).max()) and 0 < floor < 1e-5
    for s in range(S):
        for b in range(B):
            T = int(ts[b + 1] - ts[b])
            args = (g[f"{tag}_pred_logits"][s, b], g[f"{tag}_pred_masks"][s, b], g[f"{tag}_tmasks"][ts[b]:ts[b + 1]],
                    g[f"{tag}_labels"][ts[b]:ts[b + 1]], g[f"{tag}_points"][s, b], w)
            c64 = ref_matcher.cost_matrix(*args).numpy()
            ref64 = g[f"{tag}_cost_ref64"][s, b, :, :T]
            assert np.abs(c64 - ref64).max() <= 1e-12 * np.abs(ref64).max()
            c32 = ref_matcher.cost_matrix(*args, dtype=torch.float32).numpy()
            assert np.abs(c32.astype(np.float64) - ref64).max() <= 4 * floor
            want = g[f"{tag}_match"][s, b, :T]
            for C in (c64, g[f"{tag}_cost_ref32"][s, b, :, :T]):
                i, j = ref_matcher.assign(C)
                assert (np.diff(i) > 0).all() and i.tolist() == sorted(want.tolist()) and want[j].tolist() == i.tolist()
            assert (g[f"{tag}_match"][s, b, T:] == -1).all() and (g[f"{tag}_cost_ref64"][s, b, :, T:] == 0).all()


@pytest.mark.parametrize("Q,T", [(1, 1), (4, 1), (5, 3), (6, 6), (7, 6), (8, 4)])
def test_numpy_solver_against_brute_force(Q, T):
    rng = np.random.default_rng(Q * 10 + T)
    for trial in range(4):
        C = rng.standard_normal((Q, T)) * 3 if trial < 2 else rng.integers(0, 4, (Q, T)).astype(np.float64)     # ties in the second half
        q_of_t = ref_matcher.lsap(C.T)
        assert len(set(q_of_t.tolist())) == T and q_of_t.min() >= 0 and q_of_t.max() < Q
        assert abs(ref_matcher.total(C, q_of_t) - ref_matcher.brute_force_total(C)) <= 1e-12
    bad = rng.standard_normal((Q, T))
    bad[0, 0] = np.nan
    with pytest.raises(ValueError):
        ref_matcher.lsap(bad.T)
    with pytest.raises(ValueError):
        ref_matcher.lsap(np.full((T, Q), np.inf))


def test_numpy_solver_against_scipy():
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rng = np.random.default_rng(5)
    for Q, T in [(100, 19), (33, 33), (65, 64)]:
        C = rng.standard_normal((Q, T)).astype(np.float32)
        i, j = ref_matcher.assign(C)
        ri, rj = lsa(C)
        assert i.tolist() == ri.tolist() and j.tolist() == rj.tolist()


def test_workspace_query_arithmetic():
    """bytes = 4 * S*B * NC * (2*Q*TP + 2*Q + TP): TP = Tmax rounded up to 16, NC = min(16, ceil(P / 64)) point chunks
    (include/mss_hip.h); 0 for a shape the kernels do not take."""
    __import__("__graft_entry__").build()

    def q(S, B, Q, Tmax, P):
        return _lib.value("mss_m2f_match_workspace_bytes", S, B, Q, Tmax, P)

    def want(S, B, Q, Tmax, P):
        TP, NC = -(-Tmax // 16) * 16, min(16, -(-P // 64))
        return 4 * S * B * NC * (2 * Q * TP + 2 * Q + TP)
    for shape in [(10, 16, 100, 12, 12544), (1, 1, 1, 1, 1), (3, 2, 100, 5, 300), (1, 1, 100, 19, 12544), (16, 3, 128, 128, 65),
                  (1, 3, 33, 17, 64), (1, 1, 100, 16, 1025)]:
        assert q(*shape) == want(*shape), shape
    assert q(10, 16, 100, 12, 12544) == 4 * 160 * 16 * (3200 + 200 + 16)
    assert q(17, 1, 100, 12, 64) == 0 and q(1, 1, 129, 12, 64) == 0 and q(1, 1, 100, 129, 64) == 0
    assert q(1, 1, 100, 0, 64) == 0 and q(1, 1, 100, 12, 0) == 0 and q(0, 1, 100, 12, 64) == 0
