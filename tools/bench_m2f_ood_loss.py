"""loss_ood of one prediction step (criterion.py:128-138, 162-187, RCL branch): multishiftseg_amd.SetCriterion.loss_ood -- two
class_mix_upsample nodes over csrc/m2f_mix.hip and the extra loss -- against the reference formulation composed from stock torch on
the same device in the same process (softmax, sigmoid, einsum, F.interpolate, crop, torch.max; the backward through autograd). Both
sides end in the same extra loss, a cross entropy on the logits plus a hinge on the score in stock torch, so that the difference is
the class mix and its backward alone.

    python tools/bench_m2f_ood_loss.py [--out profiles/m2f_ood/bench.json] [--shape c4|eval] [--rounds 10] [--loop N]

Shapes: c4 = 16 images, Q = 100, C = 19, mask logits 176 x 176, interpolated to 704 x 704, cropped to 700 x 700; eval = 2 images,
mask logits 256 x 512 -> 1024 x 2048, no crop. The two sides alternate in one process, forward + backward, in both mask-logit
layouts, and the launches are timed apart with device events. --loop N only repeats forward + backward N times: the body to put
under `rocprofv3 --kernel-trace --stats -- python tools/bench_m2f_ood_loss.py --loop 5`. Needs a GPU.

    python tools/bench_m2f_ood_loss.py --branch margin|bce [--out profiles/m2f_ood/margin_bce.json] [--inner 10]

times the other two branches (criterion.py:140-161): the one node multishiftseg_amd.class_mix_ood_loss (csrc/m2f_mix.hip around
csrc/m2f_ood_loss.hip) against the reference's lines in stock torch -- -torch.max at the low resolution, F.interpolate with
align_corners=True, the two boolean-index gathers and their means -- on the same inputs and a 30 % random ood_mask with 255
pixels. Every timed window holds --inner calls and ends in a synchronise; the sides alternate. The run section goes to
margin_bce.md beside the JSON."""
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

from bench_m2f_match import device_ms, wall  # noqa: E402

SHAPES = {"c4": dict(B=16, hw=(176, 176), size=(704, 704), crop=(700, 700)), "eval": dict(B=2, hw=(256, 512), size=(1024, 2048), crop=(1024, 2048))}
Q, C = 100, 19
RUN_MARK = "\n## Run on "


def extra_loss(logits, score, target):
    return F.cross_entropy(logits, target, ignore_index=255) + torch.relu(score + 1.0).mean()


def torch_mix(cls, masks, size, crop, neg_max):
    m = torch.einsum("bqc,bqhw->bchw", F.softmax(cls, dim=-1)[..., :-1], masks.sigmoid())
    if not neg_max:
        m = m[:, :19]
    m = F.interpolate(m, size=size, mode="bilinear", align_corners=False)[:, :, :crop[0], :crop[1]]
    return -torch.max(m, dim=1)[0] if neg_max else m


def torch_pixel_loss(cls, masks, ood, kind, margin):
    """criterion.py:130-161 in stock torch"""
    ood_mask, id_mask = ood == 1, ood == 0
    logits = torch.einsum("bqc,bqhw->bchw", F.softmax(cls, dim=-1)[..., :-1], masks.sigmoid())
    score = -torch.max(logits, dim=1)[0]
    score = F.interpolate(score.unsqueeze(1), size=ood.shape[-2:], mode="bilinear", align_corners=True).squeeze(1)
    ood_score, id_score = score[ood_mask], score[id_mask]
    if kind == "margin":
        loss = torch.pow(id_score, 2).mean()
        if ood_mask.sum() > 0:
            loss = loss + torch.pow(torch.clamp(margin - ood_score, min=0.0), 2).mean()
    else:
        loss = F.binary_cross_entropy_with_logits(id_score, torch.zeros_like(id_score), reduction="mean")
        if ood_mask.sum() > 0:
            loss = loss + F.binary_cross_entropy_with_logits(ood_score, torch.ones_like(ood_score), reduction="mean")
    return 0.5 * loss


def pixel_main(args):
    """--branch margin | bce"""
    from multishiftseg_amd import class_mix_ood_loss
    from multishiftseg_amd import kernels as K
    from multishiftseg_amd import ood_loss as OL
    cfg = SHAPES[args.shape]
    B, (h, w), (H, W) = cfg["B"], cfg["hw"], cfg["size"]
    kind, margin = args.branch, (-0.5 if args.branch == "margin" else None)        # a margin inside the scores: part of the hinge clamps
    g = torch.Generator(device="cuda").manual_seed(0)
    cls = (torch.randn(B, Q, C + 1, device="cuda", generator=g) * 2).requires_grad_(True)
    x = (torch.randn(B, Q, h, w, device="cuda", generator=g) * 3).requires_grad_(True)
    xpm = x.detach().permute(0, 2, 3, 1).contiguous().requires_grad_(True)
    r = torch.rand(B, H, W, device="cuda", generator=g)
    ood = torch.where(r < 0.3, 1, torch.where(r > 0.95, 255, 0)).to(torch.uint8)

    def clear():
        for t in (cls, x, xpm):
            t.grad = None

    def hip(m=x, pm=False, backward=True):
        for _ in range(args.inner):
            loss = class_mix_ood_loss(cls, m, ood, kind, margin, pixel_major=pm, Q=Q)
            if backward:
                loss.backward()
                clear()

    def ref(backward=True):
        for _ in range(args.inner):
            loss = torch_pixel_loss(cls, x, ood, kind, margin)
            if backward:
                loss.backward()
                clear()

    if args.loop:
        args.inner = args.loop
        hip()
        torch.cuda.synchronize()
        return
    a, b = class_mix_ood_loss(cls, x, ood, kind, margin), torch_pixel_loss(cls, x, ood, kind, margin)
    sides = {"hip_forward_ms": lambda: hip(backward=False), "hip_forward_backward_ms": hip,
             "hip_pixel_major_forward_ms": lambda: hip(xpm, True, False), "hip_pixel_major_forward_backward_ms": lambda: hip(xpm, True),
             "torch_forward_ms": lambda: ref(False), "torch_forward_backward_ms": ref}
    times = {k: [] for k in sides}
    for rnd in range(3 + args.rounds):                              # the sides alternate; three warm-up rounds
        for k, fn in sides.items():
            t = wall(fn) / args.inner
            if rnd >= 3:
                times[k].append(t)
    res = {"device": torch.cuda.get_device_name(0), "branch": kind, "margin": margin, "shape": args.shape, "B": B, "Q": Q, "C": C, "hw": [h, w],
           "size": [H, W], "calls_per_window": args.inner, "loss_hip": float(a), "loss_torch": float(b)}
    res.update({k: statistics.median(v) for k, v in times.items()})
    res.update({k.replace("_ms", "_min_max_ms"): [min(v), max(v)] for k, v in times.items()})
    res["ratio_forward"] = res["torch_forward_ms"] / res["hip_forward_ms"]
    res["ratio_forward_backward"] = res["torch_forward_backward_ms"] / res["hip_forward_backward_ms"]
    xd, cd = x.detach(), cls.detach()
    mix, prob = K.m2f_class_mix(cd, xd)
    t = OL.ood_negmax(mix)
    _, stats, _ = OL.ood_pixel_loss(t, ood, kind, margin)
    one = torch.ones((), device="cuda")
    dmix = OL.ood_pixel_loss_backward(mix, t, ood, stats, one, kind, margin)
    res["device_ms"] = {
        "mix_forward_nchw": device_ms(lambda: K.m2f_class_mix(cd, xd), args.rounds),
        "negmax": device_ms(lambda: OL.ood_negmax(mix), args.rounds),
        "pixel_loss_forward_and_fold": device_ms(lambda: OL.ood_pixel_loss(t, ood, kind, margin), args.rounds),
        "pixel_loss_backward": device_ms(lambda: OL.ood_pixel_loss_backward(mix, t, ood, stats, one, kind, margin), args.rounds),
        "mix_backward_nchw": device_ms(lambda: K.m2f_class_mix_backward(dmix, prob, cd, xd), args.rounds)}
    res["per_call_bytes"] = {"mask_logits": B * Q * h * w * 4, "mix": B * C * h * w * 4, "t": B * h * w * 4, "ood_mask": B * H * W}
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        md = os.path.join(os.path.dirname(os.path.abspath(args.out)), "margin_bce.md")
        mark = f"{RUN_MARK}{res['device']}, branch {kind}\n"
        text = open(md).read() if os.path.exists(md) else ""
        if mark in text:                                            # one run section per branch, replaced by every run of that branch
            before, after = text.split(mark, 1)
            text = before + (RUN_MARK + after.split(RUN_MARK, 1)[1] if RUN_MARK in after else "")
        with open(md, "w") as f:
            f.write(f"{text.rstrip(chr(10))}\n{mark}\n```json\n{json.dumps(res, indent=1)}\n```\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--branch", default="RCL", choices=["RCL", "margin", "bce"])
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window (--branch margin | bce)")
    ap.add_argument("--shape", default="c4", choices=sorted(SHAPES))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--loop", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_m2f_ood_loss needs an MI355X: there is no CPU measurement path")
    if args.branch != "RCL":
        return pixel_main(args)
    from multishiftseg_amd import HungarianMatcher, SetCriterion
    from multishiftseg_amd import kernels as K
    cfg = SHAPES[args.shape]
    B, (h, w), size, crop = cfg["B"], cfg["hw"], cfg["size"], cfg["crop"]
    g = torch.Generator(device="cuda").manual_seed(0)
    rand = lambda *s: torch.randn(*s, device="cuda", generator=g)
    step = {"pred_logits": rand(B, Q, C + 1) * 2, "pred_logits_ood": rand(B, Q, C + 1) * 2, "pred_masks": rand(B, Q, h, w) * 3}
    for t in step.values():
        t.requires_grad_(True)
    step["pred_masks_ood"] = step["pred_masks"]                     # as the package's decoder returns them
    pm_step = {"pred_logits": step["pred_logits"], "pred_logits_ood": step["pred_logits_ood"],
               "pred_masks_pixel_major": step["pred_masks"].detach().permute(0, 2, 3, 1).contiguous().requires_grad_(True)}
    sem = torch.randint(0, C, (B,) + crop, device="cuda", generator=g)
    targets = [{"ood_mask": torch.zeros(size, device="cuda"), "sem_seg": sem[b]} for b in range(B)]
    crit = SetCriterion(C, HungarianMatcher(2.0, 5.0, 5.0, num_points=112), {}, 0.1, ["ood"], 112, 3.0, 0.75, "RCL", None, False).cuda()
    crit.set_extra_loss(extra_loss)

    def clear():
        for t in list(step.values()) + list(pm_step.values()):
            t.grad = None

    def hip(o=step, backward=True):
        loss = crit.loss_ood(o, targets)["loss_ood"]
        if backward:
            loss.backward()
            clear()

    def ref(backward=True):
        logits = torch_mix(step["pred_logits"], step["pred_masks"], size, crop, False)
        score = torch_mix(step["pred_logits_ood"], step["pred_masks_ood"], size, crop, True)
        loss = extra_loss(logits, score, sem.clone())
        if backward:
            loss.backward()
            clear()

    if args.loop:
        for _ in range(args.loop):
            hip()
        torch.cuda.synchronize()
        return
    sides = {"hip_forward_ms": lambda: hip(backward=False), "hip_forward_backward_ms": hip,
             "hip_pixel_major_forward_ms": lambda: hip(pm_step, False), "hip_pixel_major_forward_backward_ms": lambda: hip(pm_step),
             "torch_forward_ms": lambda: ref(False), "torch_forward_backward_ms": ref}
    times = {k: [] for k in sides}
    for r in range(3 + args.rounds):                                # the sides alternate; three warm-up rounds
        for k, fn in sides.items():
            t = wall(fn)
            if r >= 3:
                times[k].append(t)
    res = {"device": torch.cuda.get_device_name(0), "shape": args.shape, "B": B, "Q": Q, "C": C, "hw": [h, w], "size": list(size), "crop": list(crop)}
    res.update({k: statistics.median(v) for k, v in times.items()})
    res["ratio_forward"] = res["torch_forward_ms"] / res["hip_forward_ms"]
    res["ratio_forward_backward"] = res["torch_forward_backward_ms"] / res["hip_forward_backward_ms"]

    cls, x = step["pred_logits"].detach(), step["pred_masks"].detach()
    dev = {}
    for tag, m, kw in (("nchw", x, {}), ("pixel_major", pm_step["pred_masks_pixel_major"].detach(), dict(pixel_major=True, Q=Q))):
        mix, prob = K.m2f_class_mix(cls, m, **kw)
        dmix = torch.randn_like(mix)
        dev[f"mix_forward_{tag}"] = device_ms(lambda: K.m2f_class_mix(cls, m, **kw), args.rounds)
        dev[f"mix_backward_{tag}"] = device_ms(lambda: K.m2f_class_mix_backward(dmix, prob, cls, m, **kw), args.rounds)
    dlogits, dscore = torch.randn((B, C) + crop, device="cuda"), torch.randn((B,) + crop, device="cuda")
    dev["upsample_logits"] = device_ms(lambda: K.m2f_mix_upsample(mix, size, crop, "logits"), args.rounds)
    dev["upsample_neg_max"] = device_ms(lambda: K.m2f_mix_upsample(mix, size, crop, "neg_max"), args.rounds)
    dev["upsample_backward_logits"] = device_ms(lambda: K.m2f_mix_upsample_backward(mix, size, crop, dlogits=dlogits), args.rounds)
    dev["upsample_backward_neg_max"] = device_ms(lambda: K.m2f_mix_upsample_backward(mix, size, crop, dscore=dscore), args.rounds)
    logits = K.m2f_mix_upsample(mix, size, crop, "logits").requires_grad_(True)
    score = K.m2f_mix_upsample(mix, size, crop, "neg_max").requires_grad_(True)
    dev["extra_loss_forward_backward"] = device_ms(lambda: extra_loss(logits, score, sem).backward(), args.rounds)
    res["device_ms"] = dev
    n_out = B * crop[0] * crop[1]
    res["per_call_bytes"] = {"mask_logits": B * Q * h * w * 4, "mix": B * C * h * w * 4, "logits": n_out * C * 4, "score": n_out * 4}
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
