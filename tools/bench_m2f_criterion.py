"""SetCriterion of one Mask2Former train step at C4: multishiftseg_amd.SetCriterion (matching + class and sampled-mask losses of
all S steps: the matcher's two launches, three forward, two backward) against the reference formulation composed from stock torch on
the same device in the same process (criterion.py:189-205, :312-363: per step a gather of the matched maps, torch.rand, grid_sample,
topk, two more grid_samples, BCE-with-logits and dice; its backward goes through grid_sample's float atomics). Both sides use the
matching of HungarianMatcher.match_steps, so the matcher is in both times.

    python tools/bench_m2f_criterion.py [--out profiles/m2f_criterion/bench.json] [--B 16] [--S 10] [--rounds 10] [--loop N]

Shape: B = 16 images, S = 10 prediction steps, Q = 100, mask logits 176 x 176, targets 704 x 704 with 8 .. 16 masks per image,
P = 12544 points, K = 37632 candidates, k = 9408 kept. Forward and forward + backward, both mask-logit layouts, and the launches
timed apart with device events. --loop N only repeats forward + backward N times: the body to put under
`rocprofv3 --kernel-trace --stats -- python tools/bench_m2f_criterion.py --loop 5`. Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_m2f_match import device_ms, make_inputs, wall  # noqa: E402

NUM_CLASSES, EOS, OVERSAMPLE, KEEP = 19, 0.1, 3.0, 0.75
RUN_MARK = "\n## Run on "


def sample(x, pts):
    """x [N,1,H,W], pts [N,P,2] -> [N,P] (detectron2's point_sample)."""
    return F.grid_sample(x, 2.0 * pts[:, :, None, :] - 1.0, align_corners=False)[:, 0, :, 0]


def torch_composition(steps, targets, pairs, P, weight):
    """loss_labels + loss_masks per step in stock torch; pairs[s][b] = (query indices, target indices) on the device."""
    num_masks = max(sum(len(t["labels"]) for t in targets), 1)
    K, k = int(P * OVERSAMPLE), int(KEEP * P)
    out = {}
    for s, o in enumerate(steps):
        sfx = "" if s == 0 else f"_{s - 1}"
        lg, pm = o["pred_logits"], o["pred_masks"]
        tc = torch.full(lg.shape[:2], NUM_CLASSES, dtype=torch.int64, device=lg.device)
        for b, (i, j) in enumerate(pairs[s]):
            tc[b, i] = targets[b]["labels"][j]
        out["loss_ce" + sfx] = F.cross_entropy(lg.transpose(1, 2), tc, weight)
        src = torch.cat([pm[b][i] for b, (i, j) in enumerate(pairs[s])])[:, None]
        tgt = torch.cat([targets[b]["masks"][j] for b, (i, j) in enumerate(pairs[s])]).to(src)[:, None]
        with torch.no_grad():
            cand = torch.rand(src.shape[0], K, 2, device=src.device)
            idx = torch.topk(-sample(src, cand).abs(), k=k, dim=1)[1]
            pts = torch.cat([torch.gather(cand, 1, idx[:, :, None].expand(-1, -1, 2)), torch.rand(src.shape[0], P - k, 2, device=src.device)], 1)
            t = sample(tgt, pts)
        x = sample(src, pts)
        out["loss_mask" + sfx] = F.binary_cross_entropy_with_logits(x, t, reduction="none").mean(1).sum() / num_masks
        sg = x.sigmoid()
        out["loss_dice" + sfx] = (1 - (2 * (sg * t).sum(-1) + 1) / (sg.sum(-1) + t.sum(-1) + 1)).sum() / num_masks
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--B", type=int, default=16)
    ap.add_argument("--S", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--loop", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_m2f_criterion needs an MI355X: there is no CPU measurement path")
    from multishiftseg_amd import HungarianMatcher, SetCriterion
    from multishiftseg_amd import kernels as K
    Q, P = 100, 12544
    steps, targets, mpoints = make_inputs(args.B, args.S, Q, (176, 176), (704, 704), P)
    for o in steps:
        o["pred_logits"].requires_grad_(True)
        o["pred_masks"].requires_grad_(True)
    outputs = dict(steps[0], aux_outputs=steps[1:])
    matcher = HungarianMatcher(2.0, 5.0, 5.0, num_points=P)
    crit = SetCriterion(NUM_CLASSES, matcher, {}, EOS, ["labels", "masks"], P, OVERSAMPLE, KEEP, None, None, True).cuda()
    pm_steps = [{"pred_logits": o["pred_logits"], "pred_masks_pixel_major": o["pred_masks"].detach().permute(0, 2, 3, 1).contiguous().requires_grad_(True)}
                for o in steps]
    pm_outputs = dict(pm_steps[0], aux_outputs=pm_steps[1:])

    def clear():
        for o in steps + pm_steps:
            for t in o.values():
                t.grad = None

    def hip(out=outputs, backward=False):
        losses = crit(out, targets, matcher_points=mpoints)
        if backward:
            sum(losses.values()).backward()
            clear()

    def ref(backward=False):
        pairs = [[(i.cuda(), j.cuda()) for i, j in step] for step in matcher.match_steps(steps, targets, point_coords=mpoints)]
        losses = torch_composition(steps, targets, pairs, P, crit.empty_weight)
        if backward:
            sum(losses.values()).backward()
            clear()

    if args.loop:
        for _ in range(args.loop):
            hip(backward=True)
        torch.cuda.synchronize()
        return
    sides = {"hip_forward_ms": lambda: hip(), "hip_forward_backward_ms": lambda: hip(backward=True),
             "hip_pixel_major_forward_ms": lambda: hip(pm_outputs), "hip_pixel_major_forward_backward_ms": lambda: hip(pm_outputs, True),
             "torch_forward_ms": lambda: ref(), "torch_forward_backward_ms": lambda: ref(True)}
    times = {k: [] for k in sides}
    for r in range(3 + args.rounds):                                # the sides alternate; three warm-up rounds
        for k, fn in sides.items():
            t = wall(fn)
            if r >= 3:
                times[k].append(t)
    res = {"device": torch.cuda.get_device_name(0), "B": args.B, "S": args.S, "Q": Q, "P": P,
           "targets_per_image": [len(t["labels"]) for t in targets]}
    res.update({k: statistics.median(v) for k, v in times.items()})
    res["ratio_forward"] = res["torch_forward_ms"] / res["hip_forward_ms"]
    res["ratio_forward_backward"] = res["torch_forward_backward_ms"] / res["hip_forward_backward_ms"]

    tmask, tstart, labels, counts = matcher._pack_targets(targets, "cuda")
    total = sum(counts)
    n_cand, n_keep = crit.selection()[1:]
    masks = [o["pred_masks"].detach() for o in steps]
    logits = [o["pred_logits"].detach() for o in steps]
    pmm = [o["pred_masks_pixel_major"].detach() for o in pm_steps]
    match = matcher.match_steps(steps, targets, point_coords=mpoints, device_only=True)
    cand = torch.rand((args.S, total, n_cand, 2), device="cuda")
    rnd = torch.rand((args.S * total, P - n_keep, 2), device="cuda")
    scales = (1.0 / total,)
    dev = {}
    for tag, m, kw in (("nchw", masks, {}), ("pixel_major", pmm, dict(pixel_major=True, Q=Q))):
        points = K.m2f_point_select(m, tmask, tstart, match, cand, rnd, n_keep, P, **kw)
        rows = K.m2f_mask_loss(m, tmask, tstart, match, points, **kw)
        loss, tclass, bad, wsum = K.m2f_label_loss(logits, labels, tstart, match, crit.empty_weight, rows, P, scales)
        gloss = torch.ones_like(loss)
        dev[f"select_{tag}"] = device_ms(lambda: K.m2f_point_select(m, tmask, tstart, match, cand, rnd, n_keep, P, **kw), args.rounds)
        dev[f"mask_forward_{tag}"] = device_ms(lambda: K.m2f_mask_loss(m, tmask, tstart, match, points, **kw), args.rounds)
        dev[f"mask_backward_with_zero_fill_{tag}"] = device_ms(
            lambda: K.m2f_mask_loss_backward(m, tmask, tstart, match, bad, points, rows, gloss, scales, **kw), args.rounds)
    dev["label_forward_finalize"] = device_ms(lambda: K.m2f_label_loss(logits, labels, tstart, match, crit.empty_weight, rows, P, scales), args.rounds)
    dev["label_backward"] = device_ms(lambda: K.m2f_label_loss_backward(logits, tclass, bad, crit.empty_weight, wsum, gloss), args.rounds)
    dev["torch_rand_candidates"] = device_ms(lambda: torch.rand((args.S, total, n_cand, 2), device="cuda"), args.rounds)
    res["device_ms"] = dev
    R = args.S * total
    res["per_call_work"] = {"rows": R, "candidate_samples": R * n_cand, "candidate_bytes": R * n_cand * 8,
                            "transcendental_points_forward": R * P, "dense_mask_gradient_bytes": args.S * args.B * Q * 176 * 176 * 4}
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        md = os.path.join(os.path.dirname(os.path.abspath(args.out)), "bench.md")
        head = open(md).read().split(RUN_MARK)[0].rstrip("\n") + "\n" if os.path.exists(md) else ""
        with open(md, "w") as f:                                    # one run section, replaced by every run
            f.write(f"{head}{RUN_MARK}{res['device']}\n\n```json\n{json.dumps(res, indent=1)}\n```\n")


if __name__ == "__main__":
    main()
