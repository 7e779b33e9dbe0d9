"""The host reference of the OOD-metric kernels (tests/ref_ood_metric.py: rank counts in exact integers) against the restatement
of the reference's own route (oracle/metric.py: sort everything, cumulative sums): the false-positive count with ==, AUROC and AP
to 1e-15 -- on every multiset of 1..4 OOD and 1..4 inlier scores from four values at 14 recall levels (the low levels pick
recall 0 where inliers lie above every OOD score), on the reference's own golden outputs and on random maps with ties. And the
key map at the edges of float32: the keys order exactly as the scores do."""
import itertools

import numpy as np
import pytest

import ref_ood_metric as R
from conftest import golden
from oracle import metric as ometric

LEVELS = (0.0, 1e-9, 0.1, 0.125, 0.25, 0.3, 0.375, 0.5, 0.625, 0.7, 0.75, 0.875, 0.95, 1.0)
TOL = 1e-15


def multisets(values, most=4):
    return [c for k in range(1, most + 1) for c in itertools.combinations_with_replacement(values, k)]


def _compare(pos, neg, what, levels=LEVELS):
    """One (OOD scores, inlier scores) pair at every level; AUROC and AP do not depend on the level."""
    pos, neg = np.asarray(pos, dtype=np.float32), np.asarray(neg, dtype=np.float32)
    u2, ap, fps = R.measures_levels(R.score_key(pos), R.score_key(neg), levels)
    y = np.r_[np.ones(pos.size, dtype=bool), np.zeros(neg.size, dtype=bool)]
    s = np.r_[pos, neg]
    P, N = pos.size, neg.size
    for level, f in zip(levels, fps):
        fpr = ometric.fpr_at_recall(y, s, level)
        assert f / N == fpr, (what, level, f, N, fpr)
    auroc, aupr = ometric.roc_auc(y, s), ometric.average_precision(y, s)
    assert abs(u2 / (2 * P * N) - auroc) <= TOL, (what, u2 / (2 * P * N), auroc)
    assert abs(float(ap) - aupr) <= TOL, (what, float(ap), aupr)


def test_four_value_enumeration():
    sets = multisets((0.0, 1.0, 2.0, 3.0))
    assert len(sets) ** 2 * len(LEVELS) == 66654
    for pos in sets:
        for neg in sets:
            _compare(pos, neg, (pos, neg))


def test_issue_example_picks_recall_zero():
    u2, ap, fps = R.measures(R.score_key([1.0, 2.0]), R.score_key([5.0, 1.5]), 0.1)
    assert (u2, fps) == (2, 1) and fps / 2 == 0.5


def test_golden_reference_measures():
    g = golden("ood_metrics")
    tags = sorted(k[:-len("_measures")] for k in g.files if k.endswith("_measures"))
    assert tags
    for tag in tags:
        score, label = g[tag + "_score"].reshape(-1), g[tag + "_label"].reshape(-1)
        pos, neg = score[label == 1], score[label == 0]
        u2, ap, fps = R.measures(R.score_key(pos), R.score_key(neg), 0.95)
        want = g[tag + "_measures"]
        assert abs(u2 / (2 * pos.size * neg.size) - want[0]) <= TOL, tag
        assert abs(float(ap) - want[1]) <= TOL, tag
        assert fps / neg.size == want[2], tag
        _compare(pos, neg, tag)


@pytest.mark.parametrize("n,quant,ppos,seed", [(2, 1, 0.5, 0), (17, 2, 0.3, 1), (64, 1, 0.5, 2), (200, 4, 0.1, 3), (200, None, 0.8, 4)])
def test_random_with_ties(n, quant, ppos, seed):
    rng = np.random.default_rng(seed)
    label = (rng.random(n) < ppos).astype(np.int64)
    label[:2] = [1, 0]
    score = (rng.standard_normal(n) + 0.7 * label).astype(np.float32)
    if quant:
        score = (np.round(score * quant) / quant).astype(np.float32)
    _compare(score[label == 1], score[label == 0], seed)


def test_lane_layout_partitions_the_map():
    rng = np.random.default_rng(5)
    n = 9 * R.CHUNK + 5
    score = rng.standard_normal(n).astype(np.float32)
    label = rng.choice([0, 1, 255, -3], size=n)
    neg, pos, counters, cap = R.lane_layout(score, label, 0, 1)
    assert cap == 2 * R.CHUNK == R.lanes_cap(n)
    assert [c & 0xFFFFFFFF for c in counters] == [a.size for a in neg] and [c >> 32 for c in counters] == [a.size for a in pos]
    assert np.array_equal(np.sort(np.concatenate(neg)), np.sort(R.score_key(score[label == 0])))
    assert np.array_equal(np.sort(np.concatenate(pos)), np.sort(R.score_key(score[label == 1])))
    # the ninth chunk wraps to lane 0: it holds the last 5 pixels too
    tail = (label[8 * R.CHUNK:] == 0).sum() + (label[:R.CHUNK] == 0).sum()
    assert neg[0].size == tail and all(a.size + b.size <= cap for a, b in zip(neg, pos))


def test_score_key_orders_as_the_scores():
    s = R.special_scores()
    k = R.score_key(s)
    assert k.dtype == np.uint32 and s.size == 14
    for i in range(s.size):
        for j in range(s.size):
            assert (k[i] < k[j]) == (s[i] < s[j]), (s[i], s[j])
            assert (k[i] == k[j]) == (s[i] == s[j]), (s[i], s[j])
    assert k[5] == k[6] == 0x80000000                                    # -0.0 and 0.0: one key
    assert k[0] == 0x007FFFFF and k[-1] == 0xFF800000                    # -inf, inf
    assert k[4] == 0x7FFFFFFE and k[7] == 0x80000001                     # the smallest denormals keep their place
