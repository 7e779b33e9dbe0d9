"""Test helper: a restatement of HungarianMatcher's cost (lib/network/mask2former/modeling/matcher.py:105-148) in stock torch at a
chosen precision (float64 = the yardstick, float32 = the reference's own arithmetic, whose distance to float64 is the error floor
the HIP kernels are held against), and a pure-numpy shortest-augmenting-path solver for the assignment, so that no GPU test needs
scipy. Plain module, imported by the tests that want it."""
import itertools

import numpy as np
import torch
import torch.nn.functional as F


def point_sample(x, pts):
    """x [N,H,W], pts [P,2] (x, y) in [0,1) -> [N,P]: F.grid_sample(2u - 1, bilinear, align_corners=False, zero padding)."""
    if x.shape[0] == 0:
        return x.new_zeros((0, pts.shape[0]))
    grid = (2.0 * pts - 1.0)[None, :, None, :].expand(x.shape[0], -1, -1, -1)
    return F.grid_sample(x[:, None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0, :, 0]


def cost_matrix(pred_logits, pred_masks, tmasks, labels, pts, weights, dtype=torch.float64):
    """One problem: pred_logits [Q,C+1], pred_masks [Q,h,w], tmasks [T,H,W] (0/1), labels [T], pts [P,2];
    weights = (cost_class, cost_mask, cost_dice) -> C [Q,T] in `dtype`."""
    w_class, w_mask, w_dice = weights
    x = point_sample(torch.as_tensor(pred_masks).to(dtype), torch.as_tensor(pts).to(dtype))
    t = point_sample(torch.as_tensor(tmasks).to(dtype), torch.as_tensor(pts).to(dtype))
    P = x.shape[1]
    pos = torch.clamp(-x, min=0) + torch.log1p(torch.exp(-x.abs()))
    neg = x + pos
    cost_mask = (pos @ t.T + neg @ (1 - t).T) / P
    s = torch.sigmoid(x)
    cost_dice = 1 - (2 * (s @ t.T) + 1) / (s.sum(-1)[:, None] + t.sum(-1)[None, :] + 1)
    prob = torch.as_tensor(pred_logits).to(dtype).softmax(-1)
    cost_class = -prob[:, torch.as_tensor(labels).long()]
    return w_mask * cost_mask + w_class * cost_class + w_dice * cost_dice


def lsap(cost):
    """Rectangular assignment by shortest augmenting paths (Crouse 2016) in float64: cost [n_rows, n_cols], n_rows <= n_cols ->
    col4row [n_rows]. ValueError for NaN / -inf entries or an infeasible matrix, as scipy raises."""
    C = np.asarray(cost, np.float64)
    nr, nc = C.shape
    assert nr <= nc
    if np.isnan(C).any() or np.isneginf(C).any():
        raise ValueError("matrix contains invalid numeric entries")
    u, v = np.zeros(nr), np.zeros(nc)
    col4row, row4col = np.full(nr, -1), np.full(nc, -1)
    for cur in range(nr):
        sp = np.full(nc, np.inf)
        path = np.full(nc, -1)
        SR, SC = np.zeros(nr, bool), np.zeros(nc, bool)
        minval, i, sink = 0.0, cur, -1
        while sink < 0:
            SR[i] = True
            r = minval + C[i] - u[i] - v
            better = ~SC & (r < sp)
            sp[better], path[better] = r[better], i
            cand = np.where(SC, np.inf, sp)
            j = int(np.argmin(cand))                       # the lowest column wins a tie
            minval = cand[j]
            if not minval < np.inf:
                raise ValueError("cost matrix is infeasible")
            SC[j] = True
            if row4col[j] < 0:
                sink = j
            else:
                i = row4col[j]
        u[cur] += minval
        for r_ in np.nonzero(SR)[0]:
            if r_ != cur:
                u[r_] += minval - sp[col4row[r_]]
        v[SC] -= minval - sp[SC]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    return col4row


def assign(C):
    """C [Q,T] (T <= Q) -> (index_i ascending, index_j): what linear_sum_assignment(C) returns."""
    C = np.asarray(C, np.float64)
    if C.shape[1] == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    q_of_t = lsap(C.T)
    order = np.argsort(q_of_t)
    return q_of_t[order].astype(np.int64), order.astype(np.int64)


def brute_force_total(C):
    """The optimum of C [Q,T] by enumeration (T <= 6, small Q)."""
    C = np.asarray(C, np.float64)
    Q, T = C.shape
    return min(sum(C[q, m] for m, q in enumerate(qs)) for qs in itertools.permutations(range(Q), T))


def total(C, q_of_t):
    C = np.asarray(C, np.float64)
    return float(sum(C[q, m] for m, q in enumerate(q_of_t)))
