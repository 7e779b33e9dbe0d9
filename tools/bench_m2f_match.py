"""Hungarian matching of one Mask2Former train step at C4: HungarianMatcher.match_steps (multishiftseg_amd/matcher.py, two
launches and one copy for all S x B problems) against the reference formulation composed from stock torch on the same device in
the same process: per step and image grid_sample twice, the four einsums, `.cpu()` and scipy's linear_sum_assignment (matcher.py:
103-151; without scipy the assignment is left out of the baseline and the output says so).

    python tools/bench_m2f_match.py [--out profiles/m2f_match/bench.json] [--B 16] [--S 10] [--rounds 10]

Shape: B = 16 images, S = 10 prediction steps, Q = 100, mask logits 176 x 176, targets 704 x 704 with 8 .. 16 masks per image,
P = 12544 points. The two sides alternate (3 warm-up rounds, then `rounds` timed ones, median per side, wall clock around a call
that ends synchronised). The launches are also timed apart with device events: launch 1 + merge (cost only), the solve launch
alone (m2f_match_assign on the finished cost), and both layouts of the mask logits. Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

try:
    from scipy.optimize import linear_sum_assignment
except ImportError:
    linear_sum_assignment = None


def make_inputs(B, S, Q, hw, HW, P, seed=0):
    rng = np.random.default_rng(seed)
    g = torch.Generator(device="cuda").manual_seed(seed)
    (h, w), (H, W) = hw, HW
    steps = [{"pred_logits": torch.randn((B, Q, 20), device="cuda", generator=g) * 2,
              "pred_masks": torch.randn((B, Q, h, w), device="cuda", generator=g) * 3} for _ in range(S)]
    targets = []
    yy, xx = torch.meshgrid(torch.arange(H, device="cuda"), torch.arange(W, device="cuda"), indexing="ij")
    for b in range(B):
        T = int(rng.integers(8, 17))
        cy, cx = rng.uniform(0.1, 0.9, T) * H, rng.uniform(0.1, 0.9, T) * W
        r = rng.uniform(0.05, 0.3, T) * H
        masks = torch.stack([((yy - cy[m]) ** 2 + (xx - cx[m]) ** 2) < r[m] ** 2 for m in range(T)])
        targets.append({"labels": torch.from_numpy(rng.integers(0, 19, T)).cuda(), "masks": masks})
    points = torch.rand((S, B, P, 2), device="cuda", generator=g)
    return steps, targets, points


def torch_composition(steps, targets, points, weights):
    """matcher.py:103-151 in stock torch, one image of one step at a time."""
    w_class, w_mask, w_dice = weights
    out = []
    for s, o in enumerate(steps):
        per_image = []
        for b, t in enumerate(targets):
            prob = o["pred_logits"][b].softmax(-1)
            cost_class = -prob[:, t["labels"]]
            grid = (2.0 * points[s, b] - 1.0)[None, :, None, :]
            tm = t["masks"].to(o["pred_masks"])[:, None]
            om = o["pred_masks"][b][:, None]
            tm = F.grid_sample(tm, grid.expand(tm.shape[0], -1, -1, -1), align_corners=False)[:, 0, :, 0]
            om = F.grid_sample(om, grid.expand(om.shape[0], -1, -1, -1), align_corners=False)[:, 0, :, 0]
            pos = F.binary_cross_entropy_with_logits(om, torch.ones_like(om), reduction="none")
            neg = F.binary_cross_entropy_with_logits(om, torch.zeros_like(om), reduction="none")
            cost_mask = (torch.einsum("nc,mc->nm", pos, tm) + torch.einsum("nc,mc->nm", neg, 1 - tm)) / om.shape[1]
            sg = om.sigmoid()
            cost_dice = 1 - (2 * torch.einsum("nc,mc->nm", sg, tm) + 1) / (sg.sum(-1)[:, None] + tm.sum(-1)[None, :] + 1)
            C = (w_mask * cost_mask + w_class * cost_class + w_dice * cost_dice).cpu()
            per_image.append(linear_sum_assignment(C) if linear_sum_assignment is not None else C)
        out.append(per_image)
    return out


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def device_ms(fn, rounds):
    ts = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--S", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_m2f_match needs an MI355X: there is no CPU measurement path")
    from multishiftseg_amd import HungarianMatcher
    from multishiftseg_amd import kernels as K
    Q, P, weights = 100, 12544, (2.0, 5.0, 5.0)
    steps, targets, points = make_inputs(args.B, args.S, Q, (176, 176), (704, 704), P)
    m = HungarianMatcher(*weights, num_points=P)

    def hip():
        return m.match_steps(steps, targets, point_coords=points)

    def ref():
        return torch_composition(steps, targets, points, weights)
    got, want = hip(), ref()
    same = None
    if linear_sum_assignment is not None:
        same = sum(i.tolist() == ri.tolist() and j.tolist() == rj.tolist() for gs, ws in zip(got, want) for (i, j), (ri, rj) in zip(gs, ws))
    for _ in range(3):
        hip()
        ref()
    th, tr = [], []
    for _ in range(args.rounds):
        th.append(wall(hip))
        tr.append(wall(ref))
    tmask, tstart, labels, counts = m._pack_targets(targets, "cuda")
    Tmax = max(counts)
    masks, logits = [o["pred_masks"] for o in steps], [o["pred_logits"] for o in steps]
    pm = [x.permute(0, 2, 3, 1).contiguous() for x in masks]
    a = (tmask, tstart, labels, points, weights)
    cost = K.m2f_match_cost(masks, logits, *a, Tmax=Tmax)
    tcount = torch.tensor(counts, dtype=torch.int32, device="cuda")
    res = {"device": torch.cuda.get_device_name(0), "B": args.B, "S": args.S, "Q": Q, "P": P, "targets_per_image": counts,
           "scipy_in_baseline": linear_sum_assignment is not None, "problems_with_the_baselines_indices": same,
           "match_steps_ms": statistics.median(th), "match_steps_ms_min_max": [min(th), max(th)],
           "torch_composition_ms": statistics.median(tr), "torch_composition_ms_min_max": [min(tr), max(tr)],
           "device_ms": {
               "both_launches_nchw": device_ms(lambda: K.m2f_match_cost(masks, logits, *a, Tmax=Tmax, solve=True), args.rounds),
               "both_launches_pixel_major": device_ms(lambda: K.m2f_match_cost(pm, logits, *a, Tmax=Tmax, pixel_major=True, solve=True), args.rounds),
               "launch1_plus_merge_nchw": device_ms(lambda: K.m2f_match_cost(masks, logits, *a, Tmax=Tmax), args.rounds),
               "launch1_plus_merge_pixel_major": device_ms(lambda: K.m2f_match_cost(pm, logits, *a, Tmax=Tmax, pixel_major=True), args.rounds),
               "solve_launch_alone": device_ms(lambda: K.m2f_match_assign(cost, tcount), args.rounds)}}
    res["ratio"] = res["torch_composition_ms"] / res["match_steps_ms"]
    n = args.B * args.S
    res["per_call_work"] = {"softplus_sigmoid_evaluations": n * Q * P, "contraction_flop": 4 * Q * P * sum(counts) * args.S}
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
