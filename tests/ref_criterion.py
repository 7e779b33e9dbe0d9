"""Test helper: a restatement of SetCriterion's class and sampled-mask losses (lib/network/mask2former/modeling/criterion.py:189-205,
:244-407) in stock torch at a chosen precision: float64 is the yardstick, float32 the reference's own arithmetic, whose distance to
float64 is the error floor the HIP kernels are held against. Written from the formulas, differentiable by autograd. Plain module,
imported by the tests that want it."""
import torch
import torch.nn.functional as F

from ref_matcher import point_sample

CLEAN_K = 1 / 0.8            # criterion.py:374-376
CLEAN_KEEP = 0.95


def selection_keys(src, tgt, cand, mode, dtype=torch.float64):
    """src [h,w], tgt [H,W], cand [K,2] -> the K keys: "uncertain" -|x|, "clean" -BCEWithLogits(x, t)."""
    cand = torch.as_tensor(cand).to(dtype)
    x = point_sample(torch.as_tensor(src).to(dtype)[None], cand)[0]
    if mode == "uncertain":
        return -x.abs()
    assert mode == "clean"
    t = point_sample(torch.as_tensor(tgt).to(dtype)[None], cand)[0]
    return -(torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs())))


def select_points(src, tgt, cand, k, mode, dtype=torch.float64):
    """The indices (ascending) of the k candidates with the largest key. Ties go to the lowest candidate index (a stable descending
    sort; -0.0 == +0.0); a NaN key ranks below every number."""
    key = selection_keys(src, tgt, cand, mode, dtype)
    nan = key.isnan()
    order = torch.sort(torch.where(nan, torch.full_like(key, -float("inf")), key), descending=True, stable=True).indices
    late = nan[order]
    order = torch.cat([order[~late], order[late]])
    return torch.sort(order[:k]).values


def bce_with_logits(x, t):
    """softplus(x) - x t. Written with logsigmoid, whose backward is analytic: autograd gives sigmoid(x) - t at every x. The form
    clamp(x, 0) + log1p(exp(-|x|)) has the same values, but autograd takes the one-sided slopes of clamp and abs at x == 0 and
    gives 1 - t there."""
    return -F.logsigmoid(-x) - x * t


def dice_terms(x, t):
    """x, t [R,P] -> [R]: 1 - (2 sum sigmoid(x) t + 1) / (sum sigmoid(x) + sum t + 1)."""
    s = torch.sigmoid(x)
    return 1 - (2 * (s * t).sum(-1) + 1) / (s.sum(-1) + t.sum(-1) + 1)


def mask_losses(src_rows, tgt_rows, points, num_masks):
    """src_rows [R,h,w], tgt_rows [R,H,W], points [R,P,2] -> (loss_mask, loss_dice) in the dtype of src_rows."""
    dtype = src_rows.dtype
    if src_rows.shape[0] == 0:
        z = src_rows.sum() * 0
        return z, z
    x = torch.stack([point_sample(src_rows[r][None], points[r].to(dtype))[0] for r in range(src_rows.shape[0])])
    t = torch.stack([point_sample(tgt_rows[r][None].to(dtype), points[r].to(dtype))[0] for r in range(src_rows.shape[0])])
    return bce_with_logits(x, t).mean(1).sum() / num_masks, dice_terms(x, t).sum() / num_masks


def label_loss(logits, target_classes, weight):
    """logits [N,C+1], target_classes [N], weight [C+1] -> sum w[c] (logsumexp - x[c]) / sum w[c]."""
    w = weight.to(logits.dtype)[target_classes]
    nll = torch.logsumexp(logits, -1) - logits.gather(1, target_classes[:, None])[:, 0]
    return (w * nll).sum() / w.sum()


def criterion(outputs_steps, targets, match, points, num_classes, eos_coef, num_masks=None, aug=False):
    """outputs_steps: S dicts {"pred_logits" [B,Q,C+1], "pred_masks" [B,Q,h,w]} (their dtype is the arithmetic's); targets: B dicts
    {"labels" [T_b], "masks" [T_b,H,W]}; match [S,B,Tmax] (the query of target m); points [S * sum T, P, 2], row s * sum T + g.
    -> dict in SetCriterion's key order."""
    S, B = len(outputs_steps), len(targets)
    counts = [int(t["labels"].shape[0]) for t in targets]
    total = sum(counts)
    starts = [sum(counts[:b]) for b in range(B + 1)]
    dtype = outputs_steps[0]["pred_masks"].dtype
    weight = torch.ones(num_classes + 1, dtype=dtype)
    weight[-1] = eos_coef
    if num_masks is None:
        num_masks = max(total, 1)
    split = starts[B // 2]
    out = {}
    for s, o in enumerate(outputs_steps):
        sfx = "" if s == 0 else f"_{s - 1}"
        lg, pm = o["pred_logits"], o["pred_masks"]
        Q = lg.shape[1]
        tc = torch.full((B, Q), num_classes, dtype=torch.int64)
        src, tgt = [], []
        for b in range(B):
            for m in range(counts[b]):
                q = int(match[s][b][m])
                tc[b, q] = int(targets[b]["labels"][m])
                src.append(pm[b, q])
                tgt.append(torch.as_tensor(targets[b]["masks"][m]).to(dtype))
        out["loss_ce" + sfx] = label_loss(lg.reshape(B * Q, -1), tc.reshape(-1), weight)
        pts = torch.as_tensor(points)[s * total:(s + 1) * total]
        src = torch.stack(src) if src else pm.new_zeros((0,) + tuple(pm.shape[2:]))
        tgt = torch.stack(tgt) if tgt else pm.new_zeros((0, 1, 1))
        if not aug:
            out["loss_mask" + sfx], out["loss_dice" + sfx] = mask_losses(src, tgt, pts, num_masks)
        else:
            n0, n1 = split, total - split
            a = mask_losses(src[:split], tgt[:split], pts[:split], n0) if n0 else (pm.sum() * 0, pm.sum() * 0)
            c = mask_losses(src[split:], tgt[split:], pts[split:], n1) if n1 else (pm.sum() * 0, pm.sum() * 0)
            out["loss_original_mask" + sfx], out["loss_original_dice" + sfx] = 2 * a[0], 2 * a[1]
            out["loss_aug_mask" + sfx], out["loss_aug_dice" + sfx] = c[0], c[1]
    return out
