"""GPU: SetCriterion on HIP (csrc/m2f_loss.hip, multishiftseg_amd/criterion.py) against the float64 restatement of
tests/ref_criterion.py on the smallest shapes at which each mechanism can go wrong. All points are injected.

Bounds. Every loss value (each key of each step on its own), and the gradient of each step's pred_masks and pred_logits tensor, is
held to 8 x floor: its deviation (max)|hip - float64| against floor = (max)|float32 - float64| of the restatement on the same inputs,
points and matching: the bound of tests/test_gpu_matcher.py (the x8 covers another but equally sound summation order). A correctly
rounded float32 value is itself up to half an ulp from the float64 one, so the seeds
below are chosen -- on the restatement alone, on a CPU -- such that every floor of a loss value is at least 0.3 ulp of the
value (zero_map_ties excepted: its mask loss is the constant log 2, which float32 rounds correctly), and such that at most max(2, k // 100) candidates of a row lie within eps of the k-th largest key."""
import functools

import numpy as np
import pytest
import torch

import poison
import ref_criterion as ref
import ref_matcher
from multishiftseg_amd import HungarianMatcher, SetCriterion
from multishiftseg_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
HW_T = (9, 4)               # the target masks
C1 = 6                      # classes + 1
EOS = 0.1
MATCH_W = (2.0, 5.0, 5.0)
MATCH_P = 33                # the matcher's own points per image

CASES = {
    "p1_no_select": dict(S=1, B=1, Q=1, T=[1], hw=(1, 1), P=1, over=1.0, keep=0.0, seed=1),
    "p1_all_selected": dict(S=1, B=1, Q=1, T=[1], hw=(1, 1), P=1, over=1.0, keep=1.0, seed=6),
    "tb0_between": dict(S=1, B=3, Q=33, T=[4, 0, 2], hw=(1, 7), P=65, seed=1),
    "s10_q100": dict(S=10, B=3, Q=100, T=[3, 0, 5], hw=(5, 3), P=257, seed=1),
    "pm80": dict(S=1, B=1, Q=128, T=[17], hw=(5, 3), P=257, big=True, seed=9),
    "conflicts_p12544": dict(S=1, B=2, Q=100, T=[2, 1], hw=(11, 13), P=12544, seed=2),
    "zero_map_ties": dict(S=2, B=1, Q=4, T=[2], hw=(5, 3), P=65, zero=True, seed=6),
    "aug_halves": dict(S=2, B=4, Q=33, T=[2, 0, 1, 3], hw=(5, 3), P=65, aug=True, seed=1),
    "aug_empty_half": dict(S=2, B=2, Q=33, T=[0, 2], hw=(5, 3), P=65, aug=True, seed=2),
    "two_bands": dict(S=1, B=1, Q=3, T=[2], hw=(100, 80), P=257, seed=1),        # the backward's LDS window takes two passes
}


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(name, **override):
    cfg = dict(CASES[name], **override)
    c = Case()
    c.name, c.cfg = name, cfg
    rng = np.random.default_rng(1000 + cfg["seed"])
    c.S, c.B, c.Q, c.T, c.P = cfg["S"], cfg["B"], cfg["Q"], cfg["T"], cfg["P"]
    c.h, c.w = cfg["hw"]
    c.aug = cfg.get("aug", False)
    c.over, c.keep = cfg.get("over", 3.0), cfg.get("keep", 0.75)
    H, W = HW_T
    n = sum(c.T)
    c.total = n
    c.tstart = np.concatenate([[0], np.cumsum(c.T)]).astype(np.int64)
    c.tmasks = (rng.random((n, H, W)) < 0.5).astype(np.uint8)
    if n >= 2:
        c.tmasks[0] = 0                                             # an all-zero and an all-one target mask
        c.tmasks[1] = 1
    c.labels = rng.integers(0, C1 - 1, n).astype(np.int64)
    c.masks = (rng.standard_normal((c.S, c.B, c.Q, c.h, c.w)) * 3).astype(np.float32)
    if cfg.get("big"):
        c.masks = np.where(rng.random(c.masks.shape) < 0.5, np.float32(80), np.float32(-80)).astype(np.float32)
    if cfg.get("zero"):
        c.masks = np.zeros_like(c.masks)
        c.masks[1:] = np.where(rng.random(c.masks[1:].shape) < 0.5, np.float32(0.0), np.float32(-0.0))
    c.logits = (rng.standard_normal((c.S, c.B, c.Q, C1)) * 2).astype(np.float32)
    c.mpoints = rng.random((c.S, c.B, MATCH_P, 2), dtype=np.float32)
    if c.aug:
        c.mode, c.K, c.k = "clean", int(c.P * ref.CLEAN_K), int(ref.CLEAN_KEEP * c.P)
        c.sel_start = int(c.tstart[c.B // 2])
        c.Pr = c.P
    else:
        c.mode, c.K, c.k = "uncertain", int(c.P * c.over), int(c.keep * c.P)
        c.sel_start = 0
        c.Pr = c.P - c.k
    c.cand = rng.random((c.S, n - c.sel_start, c.K, 2), dtype=np.float32)
    c.rnd = rng.random((c.S * n, c.Pr, 2), dtype=np.float32)
    below1 = np.nextafter(np.float32(1), np.float32(0))
    special = [(0, 0), (0.5 / W, 0.5 / H), (0.5 / c.w, 0.5 / c.h), (below1, below1), (0, below1), (below1, 0.5 / H)]
    for j, xy in enumerate(special):                                # border taps, taps outside the map, pixel centres
        if j < c.Pr - 1:
            c.rnd[:, j] = np.array(xy, np.float32)
        if j < c.K - 1:
            c.cand[:, :, j] = np.array(xy, np.float32)
    return c


def _targets(c, device):
    return [{"labels": torch.from_numpy(c.labels[c.tstart[b]:c.tstart[b + 1]]).to(device),
             "masks": torch.from_numpy(c.tmasks[c.tstart[b]:c.tstart[b + 1]]).to(device).bool()} for b in range(c.B)]


def _ref_inputs(c, dtype, grad):
    steps = [{"pred_logits": torch.from_numpy(c.logits[s]).to(dtype).requires_grad_(grad),
              "pred_masks": torch.from_numpy(c.masks[s]).to(dtype).requires_grad_(grad)} for s in range(c.S)]
    return steps, _targets(c, "cpu")


def _coefs(keys):
    """fixed, distinct coefficients of the scalar whose gradient is taken"""
    return {k: 1.0 + 0.37 * j for j, k in enumerate(keys)}


def _criterion(c, deep=True):
    m = HungarianMatcher(*MATCH_W, num_points=MATCH_P)
    crit = SetCriterion(C1 - 1, m, {}, EOS, ["labels", "masks"], c.P, c.over, c.keep, None, None, deep,
                        mask_loss_with_pixel_selection=c.aug).to(DEV)
    crit.keep_tables = True                                         # the tests read last_points / last_match
    return crit


def _pixel_major(m, ldq):
    """NCHW [B,Q,h,w] -> [B,h,w,ldq]; the padding of the query axis holds NaN: the kernels never read it."""
    B, Q, h, w = m.shape
    out = torch.full((B, h, w, ldq), float("nan"), device=m.device)
    out[..., :Q] = m.permute(0, 2, 3, 1)
    return out


def _run_hip(c, ldq=None, masks=None, targets=None, crit=None):
    """One forward + backward of the module on the device -> dict of host tensors. ldq: the pixel-major layout with that pitch."""
    crit = _criterion(c) if crit is None else crit
    masks = c.masks if masks is None else masks
    lg = [torch.from_numpy(c.logits[s]).to(DEV).requires_grad_(True) for s in range(c.S)]
    pm = [torch.from_numpy(masks[s]).to(DEV) for s in range(c.S)]
    if ldq is not None:
        pm = [_pixel_major(m, ldq) for m in pm]
    pm = [m.requires_grad_(True) for m in pm]
    key = "pred_masks" if ldq is None else "pred_masks_pixel_major"
    steps = [{"pred_logits": a, key: b} for a, b in zip(lg, pm)]
    outputs = dict(steps[0], aux_outputs=steps[1:])
    cand = torch.from_numpy(c.cand).to(DEV) if c.k > 0 else None
    losses = crit(outputs, _targets(c, DEV) if targets is None else targets, point_candidates=cand, random_points=torch.from_numpy(c.rnd).to(DEV),
                  matcher_points=torch.from_numpy(c.mpoints).to(DEV))
    coef = _coefs(losses)
    sum(coef[k] * v for k, v in losses.items()).backward()
    gm = torch.stack([m.grad for m in pm])
    out = dict(keys=list(losses), losses=torch.stack([v.detach() for v in losses.values()]).cpu(), points=crit.last_points.cpu(),
               match=crit.last_match.cpu(), status=crit.matcher.last_status.cpu(), gl=torch.stack([a.grad for a in lg]).cpu())
    if ldq is not None:
        out["pad"] = gm[..., c.Q:].cpu()
        gm = gm[..., :c.Q].permute(0, 1, 4, 2, 3)
    out["gm"] = gm.contiguous().cpu()
    return out


@functools.lru_cache(maxsize=None)
def _restated(name, dtype):
    """The restatement at HIP's own matching and point table (recorded by the first run of the case): losses and gradients."""
    c = _case(name)
    run = _first_run(name)
    steps, targets = _ref_inputs(c, dtype, True)
    losses = ref.criterion(steps, targets, run["match"].numpy(), run["points"].to(dtype), C1 - 1, EOS, aug=c.aug)
    coef = _coefs(losses)
    sum(coef[k] * v for k, v in losses.items()).backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return dict(losses={k: float(v.detach().double()) for k, v in losses.items()}, gm=torch.stack([zero(o["pred_masks"]) for o in steps]).double(),
                gl=torch.stack([zero(o["pred_logits"]) for o in steps]).double())


@functools.lru_cache(maxsize=None)
def _first_run(name):
    return _run_hip(_case(name))


def _candidate_indices(cand, sel):
    """The candidate index of every selected point (an exact match of both coordinates)."""
    cu, pu = np.ascontiguousarray(cand).view(np.uint64)[:, 0], np.ascontiguousarray(sel).view(np.uint64)[:, 0]
    order = np.argsort(cu, kind="stable")
    idx = order[np.clip(np.searchsorted(cu[order], pu), 0, len(cu) - 1)]
    assert np.array_equal(cu[idx], pu), "a selected point is no candidate of its row"
    return idx


def check_selection(c, match, points):
    """The selection property of the module docstring, on every row; returns the rows checked."""
    checked = 0
    for s in range(c.S):
        for g in range(c.total):
            r = s * c.total + g
            b = int(np.searchsorted(c.tstart, g, side="right") - 1)
            k = c.k if g >= c.sel_start else 0
            assert np.array_equal(points[r, k:], c.rnd[r, :c.P - k]), (s, g)
            if k == 0:
                continue
            cand = c.cand[s, g - c.sel_start]
            idx = _candidate_indices(cand, points[r, :k])
            assert len(idx) == k and (np.diff(idx) > 0).all(), (s, g)           # exactly k, distinct, ascending
            if c.cfg.get("zero"):
                assert idx.tolist() == list(range(k)), (s, g)                     # all keys tie: the lowest indices win
                checked += 1
                continue
            q = int(match[s, b, g - c.tstart[b]])
            key64 = ref.selection_keys(c.masks[s, b, q], c.tmasks[g], cand, c.mode, torch.float64).numpy()
            key32 = ref.selection_keys(c.masks[s, b, q], c.tmasks[g], cand, c.mode, torch.float32).numpy().astype(np.float64)
            eps = 8 * float(np.abs(key32 - key64).max())
            tau = float(np.sort(key64)[::-1][k - 1])
            assert int((np.abs(key64 - tau) <= eps).sum()) <= max(2, k // 100), (s, g, "the check would go vacuous: choose another seed")
            chosen = np.zeros(len(cand), bool)
            chosen[idx] = True
            assert key64[chosen].min() >= tau - eps, (s, g)
            assert not (~chosen).any() or key64[~chosen].max() <= tau + eps, (s, g)
            checked += 1
    return checked


def check_values(c, run):
    """Every loss value, and the gradient of every step's pred_masks and pred_logits tensor, against its own floor."""
    r64, r32 = _restated(c.name, torch.float64), _restated(c.name, torch.float32)
    assert run["keys"] == list(r64["losses"])
    got = dict(zip(run["keys"], run["losses"].double().tolist()))
    for k in run["keys"]:
        dev, floor = abs(got[k] - r64["losses"][k]), abs(r32["losses"][k] - r64["losses"][k])
        print(f"{c.name} {k}: |hip - float64| {dev:.3e}, floor {floor:.3e}, bound {8 * floor:.3e}")
        if r64["losses"][k] == 0:                                   # the empty half of loss_masks_aug: exactly 0 by the rule
            assert got[k] == 0, k
            continue
        assert floor > 0, k
        assert dev <= 8 * floor, k
    for kind in ("gm", "gl"):
        for s in range(c.S):
            dev = float((run[kind][s].double() - r64[kind][s]).abs().max())
            floor = float((r32[kind][s] - r64[kind][s]).abs().max())
            print(f"{c.name} step {s} d/d {'pred_masks' if kind == 'gm' else 'pred_logits'}: max|hip - float64| {dev:.3e}, floor {floor:.3e}, "
                  f"bound {8 * floor:.3e}")
            assert floor > 0, (kind, s)
            assert dev <= 8 * floor, (kind, s)
    matched = torch.zeros(run["gm"].shape[:3], dtype=torch.bool)
    for s in range(c.S):
        for b in range(c.B):
            for m in range(c.T[b]):
                matched[s, b, int(run["match"][s, b, m])] = True
    assert (run["gm"][~matched] == 0).all()                         # unmatched maps are exactly 0


@pytest.mark.parametrize("name", list(CASES))
def test_case_against_the_float64_restatement(name):
    c = _case(name)
    run = _first_run(name)
    assert int(run["status"].abs().sum()) == 0
    again = _run_hip(c)
    for k in ("losses", "points", "match", "gm", "gl"):             # two runs are bit-identical
        assert torch.equal(run[k], again[k]), k
    assert torch.isfinite(run["losses"]).all() and torch.isfinite(run["gm"]).all() and torch.isfinite(run["gl"]).all()
    rows = check_selection(c, run["match"].numpy(), run["points"].numpy())
    assert rows == (c.S * (c.total - c.sel_start) if c.k else 0)
    check_values(c, run)
    for ldq in (c.Q, c.Q + 4):                                      # the decoder's layout: the same bits, the gradient in that layout
        pm = _run_hip(c, ldq=ldq)
        for k in ("losses", "points", "match", "gl", "gm"):
            assert torch.equal(run[k], pm[k]), (k, ldq)
        assert (pm["pad"] == 0).all()


def _wrapper_inputs(c):
    crit = _criterion(c)
    tm, ts, lb, _ = crit.matcher._pack_targets(_targets(c, DEV), DEV)
    masks = [torch.from_numpy(c.masks[s]).to(DEV) for s in range(c.S)]
    logits = [torch.from_numpy(c.logits[s]).to(DEV) for s in range(c.S)]
    steps = [{"pred_logits": a, "pred_masks": b} for a, b in zip(logits, masks)]
    match = crit.matcher.match_steps(steps, _targets(c, DEV), point_coords=torch.from_numpy(c.mpoints).to(DEV), device_only=True)
    return crit, tm, ts, lb, masks, logits, match


@pytest.mark.parametrize("name", list(CASES))
def test_poisoned_scratch_and_padding_change_nothing(name):
    """Two clean runs and one run under each poison of tests/poison.py are bit-identical, wrapper by wrapper and through the module:
    no workspace, padding or output element is read before it is written."""
    c = _case(name)
    crit, tm, ts, lb, masks, logits, match = _wrapper_inputs(c)
    cand, rnd = torch.from_numpy(c.cand).to(DEV) if c.k > 0 else None, torch.from_numpy(c.rnd).to(DEV)
    n0 = c.sel_start
    scales, split = ((2.0 / n0 if n0 else 0.0, 1.0 / (c.total - n0)), n0) if c.aug else ((1.0 / c.total,), None)
    weight = crit.empty_weight

    def select(m=masks, **kw):
        return K.m2f_point_select(m, tm, ts, match, cand, rnd, c.k, c.P, mode=c.mode, sel_start=c.sel_start, **kw)
    points = poison.poison_runs(select, bitwise=True)["clean"][0].to(DEV)
    assert torch.equal(points.cpu(), _first_run(name)["points"])
    padded = [_pixel_major(m, c.Q + 4) for m in masks]
    assert torch.equal(poison.poison_runs(lambda: select(padded, pixel_major=True, Q=c.Q), bitwise=True)["clean"][0], points.cpu())
    rows = poison.poison_runs(lambda: K.m2f_mask_loss(masks, tm, ts, match, points), bitwise=True)["clean"][0].to(DEV)
    assert torch.equal(poison.poison_runs(lambda: K.m2f_mask_loss(padded, tm, ts, match, points, pixel_major=True, Q=c.Q), bitwise=True)["clean"][0],
                       rows.cpu())
    out = poison.poison_runs(lambda: list(K.m2f_label_loss(logits, lb, ts, match, weight, rows, c.P, scales, split)), bitwise=True)["clean"]
    loss, tclass, bad, wsum = (t.to(DEV) for t in out)
    assert int(bad.sum()) == 0
    gloss = torch.linspace(0.5, 1.5, loss.numel(), device=DEV).view_as(loss)
    poison.poison_runs(lambda: K.m2f_mask_loss_backward(masks, tm, ts, match, bad, points, rows, gloss, scales, split), bitwise=True)
    poison.poison_runs(lambda: K.m2f_mask_loss_backward(padded, tm, ts, match, bad, points, rows, gloss, scales, split, pixel_major=True, Q=c.Q),
                       bitwise=True)
    poison.poison_runs(lambda: K.m2f_label_loss_backward(logits, tclass, bad, weight, wsum, gloss), bitwise=True)

    def module():
        run = _run_hip(c, crit=crit)
        return [run["losses"], run["points"], run["gm"], run["gl"]]
    runs = poison.poison_runs(module, bitwise=True)
    assert torch.equal(runs["clean"][0], _first_run(name)["losses"])


def test_module_end_to_end_with_deep_supervision_and_no_host_synchronisation():
    c = _case("s10_q100")
    crit = _criterion(c)
    lg = [torch.from_numpy(c.logits[s]).to(DEV).requires_grad_(True) for s in range(c.S)]
    pm = [torch.from_numpy(c.masks[s]).to(DEV).requires_grad_(True) for s in range(c.S)]
    steps = [{"pred_logits": a, "pred_masks": b} for a, b in zip(lg, pm)]
    outputs = dict(steps[0], aux_outputs=steps[1:])
    targets = _targets(c, DEV)
    inject = dict(point_candidates=torch.from_numpy(c.cand).to(DEV), random_points=torch.from_numpy(c.rnd).to(DEV),
                  matcher_points=torch.from_numpy(c.mpoints).to(DEV))
    want = ["loss_ce", "loss_mask", "loss_dice"] + [f"{k}_{i}" for i in range(c.S - 1) for k in ("loss_ce", "loss_mask", "loss_dice")]
    coef = _coefs(want)
    crit(outputs, targets, **inject)                                # a first call: lazy initialisation is not what is checked below
    torch.cuda.synchronize()
    # torch.cuda.set_sync_debug_mode exists in the ROCm build of torch too; where it does not, the property stays unchecked here
    checked = hasattr(torch.cuda, "set_sync_debug_mode")
    if checked:
        torch.cuda.set_sync_debug_mode("error")
    try:
        losses = crit(outputs, targets, **inject)
        sum(coef[k] * v for k, v in losses.items()).backward()
    finally:
        if checked:
            torch.cuda.set_sync_debug_mode("default")
    print(f"host synchronisation inside forward + backward: {'none (sync debug mode error)' if checked else 'UNCHECKED'}")
    assert list(losses) == want                                     # the reference's keys, in its order
    assert all(v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda and v.requires_grad for v in losses.values())
    run = _first_run("s10_q100")
    assert torch.equal(torch.stack([v.detach() for v in losses.values()]).cpu(), run["losses"])
    gm, gl = torch.stack([m.grad for m in pm]).cpu(), torch.stack([a.grad for a in lg]).cpu()
    assert torch.equal(gm, run["gm"]) and torch.equal(gl, run["gl"])
    check_values(c, dict(run, gm=gm, gl=gl))                        # every step's .grad against the restatement
    only_last = _criterion(c, deep=False)(outputs, targets, point_candidates=inject["point_candidates"][:1],
                                          random_points=inject["random_points"][:c.total], matcher_points=inject["matcher_points"][:1])
    assert list(only_last) == want[:3]
    assert all(torch.equal(only_last[k], losses[k]) for k in only_last)
    drawn = crit(outputs, targets)                                  # its own random numbers: finite values of the same keys
    assert list(drawn) == want and all(bool(torch.isfinite(v)) for v in drawn.values())


def test_unsolved_problems_and_bad_labels_give_nan_losses_and_zero_gradients():
    c = _case("tb0_between", S=3)
    masks = c.masks.copy()
    masks[1, 0, 5] = np.nan                                         # a NaN in the cost of problem (step 1, image 0): matcher status 1
    run = _run_hip(c, masks=masks)
    assert run["status"].tolist() == [[0, 0, 0], [1, 0, 0], [0, 0, 0]]
    losses = run["losses"].view(c.S, 3)
    assert torch.isnan(losses[1]).all() and torch.isfinite(losses[0]).all() and torch.isfinite(losses[2]).all()
    assert torch.isfinite(run["gm"]).all() and torch.isfinite(run["gl"]).all()
    assert (run["gm"][1] == 0).all() and (run["gl"][1] == 0).all()
    clean = _run_hip(c)
    for s in (0, 2):                                                # the other steps are unaffected
        assert torch.equal(losses[s], clean["losses"].view(c.S, 3)[s])
        assert torch.equal(run["gm"][s], clean["gm"][s]) and torch.equal(run["gl"][s], clean["gl"][s])
    targets = _targets(c, DEV)
    targets[2]["labels"][1] = C1 - 1                                # a label outside [0, num_classes): every step reads it
    run = _run_hip(c, targets=targets)
    assert torch.isnan(run["losses"]).all()
    assert (run["gm"] == 0).all() and (run["gl"] == 0).all()
