"""TEST INFRASTRUCTURE ONLY -- host reference of what each OOD-metric kernel of csrc/metric.hip has to produce, in numpy and Python
integers: the order-preserving key of a score, the eight-lane layout the compaction kernels leave behind, and the three measures
as functions of rank counts (u2 and fps as exact integers, AP as a fractions.Fraction). oracle/metric.py restates the reference's
own route (sort all scores, cumulative sums, trapezoids); tests/test_ood_metric_ref_cpu.py pins the two against each other."""
from fractions import Fraction

import numpy as np

LANES = 8                      # counters / key segments per map (csrc/metric.hip, oodm_compact_body)
CHUNK = 4096                   # pixels a workgroup compacts at a time


def special_scores():
    """float32 scores at the edges of the key map, ascending; -0.0 and 0.0 are one score."""
    f = np.finfo(np.float32)
    big_denormal = np.array([0x007FFFFF], dtype=np.uint32).view(np.float32)[0]
    return np.array([-np.inf, f.min, -1.0, -f.tiny, -1e-45, -0.0, 0.0, 1e-45, big_denormal, f.tiny, 1.0,
                     np.nextafter(np.float32(1), np.float32(2)), f.max, np.inf], dtype=np.float32)


def score_key(score):
    """uint32 keys that order as the float32 scores do: add +0.0 (folds -0.0 onto 0.0), then flip the sign bit of a
    non-negative score and every bit of a negative one."""
    v = np.asarray(score, dtype=np.float32) + np.float32(0.0)
    u = np.ascontiguousarray(v).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def lanes_cap(n):
    """Slots per lane segment: the lane's share of the 4096-pixel chunks, rounded up (mss_oodm_compact_lanes_cap)."""
    if n <= 0:
        return 0
    chunks = (n + CHUNK - 1) // CHUNK
    return (chunks + LANES - 1) // LANES * CHUNK


def lane_layout(score, label, id_in, id_out):
    """(neg, pos, counters, cap): per lane the ascending uint32 keys of its id_in pixels and of its id_out pixels, the packed
    counters #id_in | #id_out << 32 as Python integers, and the segment size. Pixel i lies in chunk i // 4096, lane chunk % 8."""
    score = np.asarray(score, dtype=np.float32).reshape(-1)
    label = np.asarray(label).reshape(-1)
    n = score.size
    keys = score_key(score)
    lane = (np.arange(n, dtype=np.int64) // CHUNK) % LANES
    neg, pos, counters = [], [], []
    for ln in range(LANES):
        here = lane == ln
        neg.append(np.sort(keys[here & (label == id_in)]))
        pos.append(np.sort(keys[here & (label == id_out)]))
        counters.append(int(neg[-1].size) | (int(pos[-1].size) << 32))
    return neg, pos, counters, lanes_cap(n)


def measures(pos_keys, neg_keys, recall_level):
    """(u2, ap, fps) at one recall level: measures_levels for a single level."""
    u2, ap, fps = measures_levels(pos_keys, neg_keys, (recall_level,))
    return u2, ap, fps[0]


def measures_levels(pos_keys, neg_keys, recall_levels):
    """(u2, ap, [fps per level]) of the OOD keys `pos_keys` against the inlier keys `neg_keys`:
      u2  = sum over the positives of 2 #neg< + #neg==, a Python integer: AUROC = u2 / (2 P N);
      ap  = 1/P sum over the positives of #pos>= / (#pos>= + #neg>=), a Fraction;
      fps = #neg >= t at the threshold t the reference picks for a recall level (lib/utils/metric.py:87-127): thresholds are the
            distinct scores of BOTH classes, descending, up to the first that reaches recall 1; the reference walks them from there
            back to the largest score and takes the first minimum of |recall - level| in float64 -- so among equal recalls
            the lowest threshold, among equal distances the higher recall, and recall 0 where inliers lie above every positive."""
    pos = np.sort(np.asarray(pos_keys, dtype=np.uint32).reshape(-1))
    neg = np.sort(np.asarray(neg_keys, dtype=np.uint32).reshape(-1))
    P, N = int(pos.size), int(neg.size)
    if P < 1 or N < 1:
        raise ValueError("measures: both classes need a key")
    below = np.searchsorted(neg, pos, side="left").astype(np.int64)
    upto = np.searchsorted(neg, pos, side="right").astype(np.int64)
    u2 = int(np.sum(below + upto, dtype=np.int64))                       # 2 #neg< + #neg== = #neg< + #neg<=
    vals, first, count = np.unique(pos, return_index=True, return_counts=True)
    neg_ge = N - np.searchsorted(neg, vals, side="left")
    ap = Fraction(0)
    for f, c, g in zip(first.tolist(), count.tolist(), neg_ge.tolist()):
        tps = P - f
        ap += Fraction(c * tps, tps + g)
    ap /= P
    thr = np.unique(np.concatenate((pos, neg)))[::-1]                   # distinct scores, descending
    tps = P - np.searchsorted(pos, thr, side="left")
    fpc = N - np.searchsorted(neg, thr, side="left")
    last = int(np.argmax(tps == P))                                      # first threshold that reaches recall 1
    recall, fpc = tps[last::-1].astype(np.float64) / np.float64(P), fpc[last::-1]
    fps = [int(fpc[int(np.argmin(np.abs(recall - np.float64(level))))]) for level in recall_levels]
    return u2, ap, fps
