"""GPU: the stage-2 optimizer of Mask2Former on HIP (multishiftseg_amd/optim.py AdamW -> mss_adamw_clip_step_f32, csrc/m2f_optim.hip)
and the step around it (multishiftseg_amd/m2f_trainer.py).

Bounds of the parity tests. The yardstick is stock torch in float32 on the CPU -- clip_grad_norm_(foreach=False) followed by
torch.optim.AdamW(foreach=False) -- measured against the float64 restatement of tests/ref_adamw.py on the same inputs. Per tensor,
the HIP parameters and both moments after the six steps may differ from float64 by at most 8 x torch's own max-abs distance from
float64 for that tensor (8 x: the project's margin for a float32 floor, tests/test_gpu_class_mix.py), and never less than
(that tensor's own step count) x np.spacing(max|value|), for the tensors where torch happens to be exact. The norm of every step likewise: 8 x torch's
error against float64, at least one float32 spacing. The worst ratios are appended to
m2f_optim_parity.json in the report directory (test_reports/ in the tree, or what MSS_REPORT_DIR names)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import ref_adamw as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 4            # chosen on the float64 restatement alone: two steps clip below 0.5, three non-zero steps do not clip


def _geometry():
    from multishiftseg_amd import _lib
    return (_lib.value("mss_adamw_chunk_elems"), _lib.value("mss_adamw_tensors_per_launch"), _lib.value("mss_adamw_blocks_per_launch"))


@functools.lru_cache(maxsize=None)
def _case(clip):
    """Inputs, the float64 outcome and stock torch's float32 outcome of the six-step sequence: computed once, never changed."""
    sizes = R.parity_sizes(*_geometry())
    case = R.parity_case(sizes, seed=SEED, clip=clip)
    case["torch"] = R.torch_cpu_run(case["p0"], case["lrs"], case["wds"], case["grads"], max_norm=case["max_norm"])
    return case


GRAD_VIEW, PARAM_VIEW = 7, 9        # tensor 7's gradient and tensor 9's parameter sit at float offset 1 of a larger buffer


def _offset_view(a):
    buf = torch.zeros(a.size + 5, device=DEV)
    view = buf[1:1 + a.size]
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4
    return view


def _run_hip(case, scratch_fill=None):
    """The six steps through optim.AdamW -> final params / moments (host), per-step norms (host), launches per step."""
    from multishiftseg_amd.optim import AdamW, adamw_plan
    ps = [torch.nn.Parameter(_offset_view(a) if i == PARAM_VIEW else torch.from_numpy(a.copy()).to(DEV)) for i, a in enumerate(case["p0"])]
    opt = AdamW([{"params": [p], "lr": lr, "weight_decay": wd} for p, lr, wd in zip(ps, case["lrs"], case["wds"])], max_norm=case["max_norm"])
    if scratch_fill is not None:                                         # poisoned from the first step on
        opt._scratch = torch.full((len(adamw_plan(case["sizes"])),), scratch_fill, device=DEV)
    norms, launches, moved = [], [], [0.0] * len(ps)
    for row in case["grads"]:
        for i, (p, g) in enumerate(zip(ps, row)):
            p.grad = None if g is None else (_offset_view(g) if i == GRAD_VIEW else torch.from_numpy(g).to(DEV))
        if scratch_fill is not None and opt._scratch is not None:
            opt._scratch.fill_(scratch_fill)
        before = [p.detach().clone() for p in ps]
        kept = [None if p.grad is None else p.grad.clone() for p in ps]
        norms.append(opt.step())
        launches.append(opt.last_launches)
        for i, p in enumerate(ps):
            if kept[i] is not None:
                assert torch.equal(p.grad, kept[i])                       # p.grad keeps the unclipped values
                moved[i] = max(moved[i], float((p.detach() - before[i]).abs().max()))
    out = dict(p=[p.detach().cpu().numpy() for p in ps], m=[opt.state[id(p)][0].cpu().numpy() for p in ps],
               v=[opt.state[id(p)][1].cpu().numpy() for p in ps], norms=[None if n is None else n.cpu().numpy().copy() for n in norms],
               launches=launches, moved=moved, steps=[opt.step_counts[id(p)] for p in ps], opt=opt)
    return out


@functools.lru_cache(maxsize=None)
def _first_run(clip):
    return _run_hip(_case(clip))


def _check_parity(case, run, report, tag):
    """Fills the report with the worst deviation / bound per quantity; returns the (quantity, tensor) pairs over their bound."""
    tp, tm, tv, _ = case["torch"][-1]
    ref = case["ref"]
    bad = []
    for kind, got, tor, want in (("param", run["p"], tp, ref.p), ("exp_avg", run["m"], tm, ref.m), ("exp_avg_sq", run["v"], tv, ref.v)):
        worst = 0.0
        for i in range(len(want)):
            floor = float(np.abs(tor[i].astype(np.float64) - want[i]).max())
            bound = max(8 * floor, ref.t[i] * float(np.spacing(np.float32(np.abs(want[i]).max()))))      # the steps THIS tensor took
            dev = float(np.abs(got[i].astype(np.float64) - want[i]).max())
            worst = max(worst, dev / bound)
            print(f"{tag} {kind}[{i}] n={want[i].size}: |hip - float64| {dev:.3e}, torch floor {floor:.3e}, bound {bound:.3e}")
            if not dev <= bound:
                bad.append((tag, kind, i, dev, bound))
        report[f"{tag}_{kind}_worst_ratio_to_bound"] = worst
    return bad


def _write_report(report):
    out = os.environ.get("MSS_REPORT_DIR") or os.path.join(ROOT, "test_reports")
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "m2f_optim_parity.json"), "a") as f:
            f.write(json.dumps(report, sort_keys=True) + "\n")
    except OSError:
        pass


def test_parity_with_clipping_over_six_steps():
    from multishiftseg_amd.optim import adamw_launches, adamw_plan
    chunk, tensors, blocks = _geometry()
    case = _case(True)
    sizes = case["sizes"]
    assert len(sizes) == tensors + 3 and max(sizes) > blocks * chunk and {1, 3, 4, 5, 255, 256, 257, chunk - 1, chunk, chunk + 1} <= set(sizes)
    assert len({(lr, wd) for lr, wd in zip(case["lrs"], case["wds"])}) == 3 and (1e-5, 0.05) in zip(case["lrs"], case["wds"])
    assert sum(1 for c in case["coefs"] if c < 0.5) >= 2                              # the clip path ...
    assert sum(1 for n in case["norms"] if 0 < n < 0.5 * case["max_norm"]) >= 1       # ... and the clamp
    assert case["norms"][R.ZERO_STEP] == 0.0 and case["coefs"][R.ZERO_STEP] == 1.0
    run = _first_run(True)
    report = {}
    bad = _check_parity(case, run, report, "clip")
    worst = 0.0
    for k in range(R.STEPS):
        want = case["norms"][k]
        floor = abs(float(case["torch"][k][3]) - want)
        bound = max(8 * floor, float(np.spacing(np.float32(want))))
        dev = abs(float(run["norms"][k]) - want)
        worst = max(worst, dev / bound)
        print(f"step {k}: norm float64 {want:.9g}, |hip - float64| {dev:.3e}, torch floor {floor:.3e}, bound {bound:.3e}, coef {case['coefs'][k]:.4g}")
    report["clip_norm_worst_ratio_to_bound"] = worst
    _write_report(report)
    assert not bad, bad
    for k in range(R.STEPS):
        want = case["norms"][k]
        bound = max(8 * abs(float(case["torch"][k][3]) - want), float(np.spacing(np.float32(want))))
        assert run["norms"][k].shape == () and abs(float(run["norms"][k]) - want) <= bound, k
    assert float(run["norms"][R.ZERO_STEP]) == 0.0
    # the all-zero step moved parameters by the decoupled decay alone; the tensor without gradients kept its own count
    none = case["none_tensor"]
    assert run["steps"] == [R.STEPS - len(R.NONE_STEPS) if i == none else R.STEPS for i in range(len(sizes))]
    for i, lr in enumerate(case["lrs"]):                                               # non-vacuity
        assert run["moved"][i] > 0.5 * lr and case["moved"][i] > 0.5 * lr, (i, run["moved"][i], lr)
    # launches: every step, the planner's prediction for the tensors that had a gradient
    for k, row in enumerate(case["grads"]):
        live = [s for s, g in zip(sizes, row) if g is not None]
        assert run["launches"][k] == adamw_launches(live, clip=True), k
    assert len({l for l, *_ in adamw_plan(sizes)}) >= 3


def test_shared_coefficient_is_bit_identical_across_elements_and_launches():
    from multishiftseg_amd.optim import AdamW, adamw_plan
    _, tensors, _ = _geometry()
    n, c = tensors + 4, 0.37
    ps = [torch.nn.Parameter(torch.zeros(1000, device=DEV)) for _ in range(n)]
    assert {l for l, _, t, *_ in adamw_plan([1000] * n) if t in (0, n - 1)} == {0, 1}      # first and last tensor: different launches
    for p in ps:
        p.grad = torch.full((1000,), c, device=DEV)
    opt = AdamW(ps, lr=1e-3, weight_decay=0.0, max_norm=1e-3)
    norm = opt.step()
    np.testing.assert_allclose(float(norm), c * np.sqrt(1000 * n), rtol=1e-6)
    first = [ps[0].detach()[0], opt.state[id(ps[0])][0][0], opt.state[id(ps[0])][1][0]]
    assert float(first[0]) != 0 and float(first[1]) != 0 and float(first[2]) != 0
    # the coefficient torch itself forms on the CPU from this norm (a Python float over a tensor: reciprocal, then product), and
    # m = lerp(0, g * coef, 1 - b1) with g * coef rounded to one float32 first
    coef = torch.clamp(1e-3 / (norm.cpu() + 1e-6), max=1.0)
    want_m = torch.zeros(()).lerp_(torch.tensor(c) * coef, 1 - 0.9)
    assert float(first[1]) == float(want_m), (float(first[1]), float(want_m), float(coef))
    for p in (ps[0], ps[-1]):
        for t, want in zip((p.detach(), *opt.state[id(p)]), first):
            assert bool((t.view(torch.int32) == want.view(torch.int32)).all())
    # a second step under torch's sync debug mode: no host synchronisation, no device-to-host copy
    torch.cuda.synchronize()
    checked = hasattr(torch.cuda, "set_sync_debug_mode")
    if checked:
        torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()
    finally:
        if checked:
            torch.cuda.set_sync_debug_mode("default")
    print(f"host synchronisation inside step(): {'none (sync debug mode error)' if checked else 'UNCHECKED'}")


def test_two_runs_are_bit_identical_whatever_the_scratch_holds():
    case = _case(True)
    nan, zero = _run_hip(case, scratch_fill=float("nan")), _run_hip(case, scratch_fill=0.0)
    first = _first_run(True)
    assert nan["opt"]._scratch is not None and nan["opt"]._scratch.dtype == torch.float32
    for other in (zero, first):
        for kind in ("p", "m", "v", "norms"):
            for a, b in zip(nan[kind], other[kind]):
                assert np.array_equal(a.view(np.int32), b.view(np.int32)), kind
    assert all(np.isfinite(a).all() for a in nan["p"])


def test_without_clipping_is_plain_adamw():
    from multishiftseg_amd.optim import adamw_launches
    case = _case(False)
    assert case["max_norm"] is None
    run = _first_run(False)
    assert all(n is None for n in run["norms"])                                        # step() returns None
    report = {}
    bad = _check_parity(case, run, report, "noclip")
    _write_report(report)
    assert not bad, bad
    clipped = _first_run(True)
    for k, row in enumerate(case["grads"]):
        live = [s for s, g in zip(case["sizes"], row) if g is not None]
        per_stage = adamw_launches(live, clip=False)
        assert run["launches"][k] == per_stage and clipped["launches"][k] == 2 * per_stage + 1, k    # the norm launches are absent
    assert run["opt"]._scratch is None


def test_a_nan_gradient_propagates_as_in_torch():
    from multishiftseg_amd.optim import AdamW
    rng = np.random.default_rng(3)
    sizes = [5, 300, 5000, 17]
    p0 = [rng.standard_normal(s).astype(np.float32) for s in sizes]
    grads = [rng.standard_normal(s).astype(np.float32) for s in sizes]
    grads[2][4321] = np.nan
    grads[3] = None
    tor = R.torch_cpu_run(p0, [1e-3] * 4, [0.01] * 4, [grads], max_norm=1.0)[0]
    assert np.isnan(tor[3]) and all(np.isnan(tor[0][i]).all() for i in range(3)) and np.array_equal(tor[0][3], p0[3])
    ps = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(DEV)) for a in p0]
    for p, g in zip(ps, grads):
        p.grad = None if g is None else torch.from_numpy(g).to(DEV)
    opt = AdamW(ps, lr=1e-3, weight_decay=0.01, max_norm=1.0)
    norm = opt.step()
    assert bool(torch.isnan(norm))
    assert all(bool(torch.isnan(p).all()) for p in ps[:3])
    assert torch.equal(ps[3].detach().cpu(), torch.from_numpy(p0[3])) and id(ps[3]) not in opt.state


class _LogitsHead(torch.nn.Module):
    """A stand-in head: its two parameters ARE the stacked class logits and mask logits of S prediction steps."""

    def __init__(self, logits, masks):
        super().__init__()
        self.logits, self.masks = torch.nn.Parameter(logits.clone()), torch.nn.Parameter(masks.clone())

    def forward(self):
        steps = [{"pred_logits": self.logits[s], "pred_masks": self.masks[s]} for s in range(self.logits.shape[0])]
        return dict(steps[0], aux_outputs=steps[1:])


def test_train_step_equals_the_steps_done_by_hand():
    import test_gpu_criterion as TC
    from multishiftseg_amd import HungarianMatcher, M2FTrainStep, SetCriterion, weighted_losses
    from multishiftseg_amd.optim import AdamW
    c = TC._case("tb0_between", S=2)
    weight_dict = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice_0": 3.0, "loss_mask_0": 0.5}      # no loss_dice, no loss_ce_0
    crit = SetCriterion(TC.C1 - 1, HungarianMatcher(*TC.MATCH_W, num_points=TC.MATCH_P), weight_dict, TC.EOS, ["labels", "masks"], c.P, c.over,
                        c.keep, None, None, True).to(DEV)
    inject = dict(point_candidates=torch.from_numpy(c.cand).to(DEV), random_points=torch.from_numpy(c.rnd).to(DEV),
                  matcher_points=torch.from_numpy(c.mpoints).to(DEV))
    targets = TC._targets(c, DEV)
    logits, masks = torch.from_numpy(c.logits).to(DEV), torch.from_numpy(c.masks).to(DEV)

    def make():
        head = _LogitsHead(logits, masks)
        return head, AdamW([{"params": [head.logits], "lr": 1e-3, "weight_decay": 0.05}, {"params": [head.masks], "lr": 1e-2, "weight_decay": 0.0}],
                           max_norm=0.01)
    head, opt = make()
    got, norm = M2FTrainStep(head, crit, opt)(targets=targets, **inject)
    hand, hopt = make()
    raw = crit(hand(), targets, **inject)
    weighted = weighted_losses(raw, weight_dict)
    sum(weighted.values()).backward()
    grads = [hand.logits.grad.clone(), hand.masks.grad.clone()]
    hnorm = hopt.step()
    assert list(got) == ["loss_ce", "loss_mask", "loss_mask_0", "loss_dice_0"] and set(raw) - set(got) == {"loss_dice", "loss_ce_0"}
    for k, v in got.items():
        assert not v.requires_grad and torch.equal(v, (raw[k] * weight_dict[k]).detach()), k
    assert torch.equal(norm, hnorm) and float(norm) > 0.01                              # the step clipped
    for a, b in ((head.logits, hand.logits), (head.masks, hand.masks)):
        assert torch.equal(a.detach(), b.detach()) and not torch.equal(a.detach(), logits if a is head.logits else masks)
        for s, t in zip(opt.state[id(a)], hopt.state[id(b)]):
            assert torch.equal(s, t)
    # a key missing from weight_dict contributes no gradient: the gradient of the listed keys alone, written out
    third, _ = make()
    raw3 = crit(third(), targets, **inject)
    sum([raw3[k] * weight_dict[k] for k in raw3 if k in weight_dict]).backward()
    assert torch.equal(third.logits.grad, grads[0]) and torch.equal(third.masks.grad, grads[1])
    assert bool((grads[0][1] == 0).all()) and bool((grads[0][0] != 0).any())              # loss_ce_0 has no weight: step 1's class logits get nothing


def test_train_step_through_the_real_decoder():
    """One stage-2 step of the trainable GMA decoder at its smallest legal configuration, with labels, masks and loss_ood (so that
    class_embed2 is reached too): finite losses, a finite positive norm, every parameter but fusion_layer moved."""
    import ref_transformer_decoder as RT
    from multishiftseg_amd import (HungarianMatcher, M2FTrainStep, MultiScaleMaskedTransformerDecoder_GMA, SetCriterion, build_m2f_optimizer,
                                   m2f_weight_dict)
    from multishiftseg_amd.loss import RelContrastiveLoss
    B, Q, C, layers = 2, 8, 19, 1
    m = MultiScaleMaskedTransformerDecoder_GMA(256, True, num_classes=C, hidden_dim=256, num_queries=Q, nheads=8, dim_feedforward=80,
                                               dec_layers=layers, pre_norm=False, mask_dim=80, enforce_input_project=False)
    m.load_state_dict(RT.synth_state_dict(41, num_layers=layers, num_queries=Q, dim_feedforward=80, mask_dim=80), strict=True)
    m = m.cuda().eval().set_trainable()
    x, feat = RT.synth_inputs(411, B, [(4, 4), (8, 8), (16, 16)], (32, 32), mask_dim=80)
    xs, ft = [torch.from_numpy(v).cuda() for v in x], torch.from_numpy(feat).cuda()
    rng = np.random.default_rng(5)
    size, crop = (64, 64), (61, 61)
    sem = rng.integers(0, C, (B,) + crop).astype(np.int64)
    sem[:, :4, :] = 255
    sem[1, 20:30, 10:40] = 254                                      # an OOD object in the augmented image
    targets = [{"labels": torch.tensor([3, 7 + b], device=DEV), "masks": torch.from_numpy(rng.random((2, 24, 24)) < 0.5).to(DEV),
                "ood_mask": torch.zeros(size, device=DEV), "sem_seg": torch.from_numpy(sem[b]).to(DEV)} for b in range(B)]
    weight_dict = m2f_weight_dict(2.0, 5.0, 5.0, 1.0, layers + 1, True)
    crit = SetCriterion(C, HungarianMatcher(2.0, 5.0, 5.0, num_points=33), weight_dict, 0.1, ["labels", "masks", "ood"], 65, 3.0, 0.75, "RCL", None,
                        True).to(DEV)
    crit.set_extra_loss(RelContrastiveLoss({"ce_weights": [50, 10], "conduct_pixel_selection": False, "inoutaug_contras_margins_tri": [10, 5, 5]},
                                           pairing="reference"))
    opt = build_m2f_optimizer(m, base_lr=1e-5, weight_decay=0.05, clip_value=0.01)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    torch.manual_seed(5)
    losses, norm = M2FTrainStep(m, crit, opt)(xs, ft, targets=targets)
    # one layer: the decoder pairs aux step j with the OOD heads of layer j, so its aux list has dec_layers - 1 = 0 entries
    assert list(losses) == ["loss_ce", "loss_mask", "loss_dice", "loss_ood"]
    assert all(bool(torch.isfinite(v)) for v in losses.values()), losses
    assert bool(torch.isfinite(norm)) and float(norm) > 0
    for n, p in m.named_parameters():
        if "fusion_layer" in n:
            assert torch.equal(p.detach(), before[n]) and id(p) not in opt.state and p.grad is None, n
        else:
            assert id(p) in opt.state and not torch.equal(p.detach(), before[n]), n
            assert bool(torch.isfinite(p).all()), n
