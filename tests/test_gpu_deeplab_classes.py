"""DeepWV3Plus on label spaces other than the 19 Cityscapes classes (12 and 33): the whole model against the class-count-free
oracles (oracle/deepv3.py, oracle/deepv3_torch.py -- both pinned to the reference at 19 by tests/test_oracle_golden.py), one
optimisation step of either stage, and the evaluation sweep."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

HEAD_SETS = ("aspp", "bot_fine", "bot_aspp", "ood_head")          # the stage-2 trainable set (exps/DeepLab.yaml:10-11)


@pytest.fixture(scope="module", params=[12, 33])
def net(request):
    """(C, params, model): synthetic weights for C classes, loaded into the HIP model."""
    from multishiftseg_amd import synth
    from multishiftseg_amd.deepv3 import DeepWV3Plus
    C = request.param
    params = synth.deepwv3plus_params(100 + C, num_classes=C)
    m = DeepWV3Plus(C)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()}, strict=True)
    for p in m.parameters():
        p.requires_grad_(False)
    return C, params, m.cuda()


def dropout_masks(n, seed=5):
    rng = np.random.default_rng(seed)
    return {"mod6": ((rng.random((n, 1024)) >= 0.3) / 0.7).astype(np.float32),
            "mod7": ((rng.random((n, 2048)) >= 0.5) / 0.5).astype(np.float32)}


@pytest.mark.parametrize("n,h,w,train", [(1, 90, 150, False), (3, 72, 104, False), (2, 70, 70, True)])
def test_forward_vs_oracle(net, n, h, w, train):
    """Two of the ragged eval sizes and the train-mode size of test_forward_vs_oracle_ragged_sizes, with its bar (1e-3)."""
    from multishiftseg_amd import kernels as K, synth
    from oracle import deepv3 as odeepv3
    C, params, model = net
    img = synth.synth_image(11, n, h, w)
    masks = dropout_masks(n) if train else None
    saved = {k: v.detach().clone() for k, v in model.state_dict().items()}
    try:
        model.train(train)
        model.dropout_masks = {k: torch.from_numpy(v) for k, v in masks.items()} if train else None
        with torch.no_grad():
            score, logit = model(torch.from_numpy(img).cuda())
            if not train:                              # the form evaluate() uses, here with the logits written as well
                with K.batched_counters():
                    x, m2 = model._run_trunk(torch.from_numpy(img).cuda())
                    s2, l2, label = model._head_forward(x, m2, (h, w), want_logit=True, want_label=True)
        rs, rl = odeepv3.forward(params, img, train=train, drop_masks=masks)
        assert tuple(logit.shape) == (n, C, h, w) and tuple(score.shape) == (n, h, w)
        print(f"C={C} {n}x{h}x{w} train={train}: max |logit - oracle| {np.abs(logit.cpu().numpy() - rl).max():.3e}, "
              f"max |score - oracle| {np.abs(score.cpu().numpy() - rs).max():.3e}")
        assert np.abs(logit.cpu().numpy() - rl).max() < 1e-3
        assert np.abs(score.cpu().numpy() - rs).max() < 1e-3
        if not train:      # with want_label: the uint8 map is the argmax of the logits the same call returns
            assert label.dtype == torch.uint8 and torch.equal(s2, score) and torch.equal(l2, logit)
            np.testing.assert_array_equal(label.cpu().numpy(), l2.cpu().numpy().argmax(1))
    finally:
        model.dropout_masks = None
        model.load_state_dict(saved)
        model.eval()


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / (np.sqrt((b ** 2).sum()) + 1e-300))


def test_gradients_vs_float64_autograd(net):
    """Gradients of the stage-2 trainable set and of final.6.weight for the linear functional sum(score * gs) + sum(logit * gl),
    2 x 3 x 70 x 70, injected Dropout2d masks, against autograd of oracle.deepv3_torch.forward_t in float64. Per tensor, in
    relative L2 (one ReLU-threshold flip does not decide it): the float32 run of the same torch oracle against its float64 run is
    the floor, and the HIP path is allowed 8 x that floor -- the project's margin for an equally sound summation order. The floor
    and the measured error of every tensor go to deeplab_classes_grads_C<C>.json in the report directory (test_reports/ in the tree,
    or what MSS_REPORT_DIR names) before anything is asserted."""
    from multishiftseg_amd import synth
    from oracle import deepv3_torch as odt
    C, params, model = net
    n, h, w = 2, 70, 70
    img = synth.synth_image(11, n, h, w)
    masks = dropout_masks(n)
    rng = np.random.default_rng(17)
    gs = rng.standard_normal((n, h, w), dtype=np.float32)
    gl = rng.standard_normal((n, C, h, w), dtype=np.float32)
    names = [k for k, _ in model.named_parameters() if any(s in k for s in HEAD_SETS)] + ["final.6.weight"]

    def oracle_grads(dtype):
        p = odt.to_torch(params, dtype)
        for k in names:
            p[k].requires_grad_(True)
        dm = {k: torch.from_numpy(v).to(dtype) for k, v in masks.items()}
        score, logit = odt.forward_t(p, torch.from_numpy(img).to(dtype), True, dm)
        f = (score * torch.from_numpy(gs).to(dtype)).sum() + (logit * torch.from_numpy(gl).to(dtype)).sum()
        return dict(zip(names, (g.numpy() for g in torch.autograd.grad(f, [p[k] for k in names]))))
    g64, g32 = oracle_grads(torch.float64), oracle_grads(torch.float32)
    saved = {k: v.detach().clone() for k, v in model.state_dict().items()}
    named = dict(model.named_parameters())
    try:
        for k, p in named.items():
            p.requires_grad_(k in names)
            p.grad = None
        model.train()
        model.dropout_masks = {k: torch.from_numpy(v) for k, v in masks.items()}
        sunk = []
        model.grad_sink = lambda k, v: sunk.append((k, tuple(v.shape)))      # the data-parallel hook sees every gradient once
        score, logit = model(torch.from_numpy(img).cuda())
        torch.autograd.backward((score, logit), (torch.from_numpy(gs).cuda(), torch.from_numpy(gl).cuda()))
        got = {k: named[k].grad.detach().cpu().numpy() for k in names}
        assert sorted(sunk) == sorted((k, tuple(named[k].shape)) for k in names)
    finally:
        model.grad_sink = None
        model.dropout_masks = None
        for p in named.values():
            p.requires_grad_(False)
            p.grad = None
        model.load_state_dict(saved)
        model.eval()
    report = {k: dict(floor=rel_l2(g32[k], g64[k]), hip=rel_l2(got[k], g64[k])) for k in names}
    for k, r in report.items():
        r["ratio"] = r["hip"] / max(r["floor"], 1e-300)
        print(f"C={C} {k}: float32 oracle vs float64 {r['floor']:.3e}, HIP vs float64 {r['hip']:.3e}, ratio {r['ratio']:.2f}")
    out = os.environ.get("MSS_REPORT_DIR") or os.path.join(ROOT, "test_reports")
    try:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, f"deeplab_classes_grads_C{C}.json"), "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
    except OSError:
        pass
    over = {k: r for k, r in report.items() if not r["hip"] <= 8 * r["floor"]}
    assert not over, over


def test_graphed_eval_replays_the_eager_forward(net):
    """trainer.GraphedEval at another class count: the captured forward gives the eager forward's bits, logits and score-only."""
    from multishiftseg_amd import synth
    from multishiftseg_amd.trainer import GraphedEval, ood_scores
    C, _, model = net
    model.eval()
    imgs = [torch.from_numpy(synth.synth_image(s, 1, 64, 96)).cuda() for s in (3, 4)]
    with torch.no_grad():
        ge = GraphedEval(model, imgs[0].shape)
        for img in imgs:
            want_s, want_l = ood_scores(model, img)
            got_s, got_l = ge(img)
            assert tuple(got_l.shape) == (1, C, 64, 96)
            assert torch.equal(got_s, want_s) and torch.equal(got_l, want_l)
        got_s, none = GraphedEval(model, imgs[0].shape, score_only=True)(imgs[1])
        assert none is None and torch.equal(got_s, ood_scores(model, imgs[1])[0])


@pytest.mark.parametrize("stage", [1, 2])
def test_train_step_at_12_classes(stage):
    """One TrainStep of either stage on two 64 x 64 pairs: a finite loss that equals oracle.loss.rel_contrastive_loss on the
    step's own logits and score with the same permutations (rtol 1e-5, what tests/test_gpu_loss.py asks of that comparison), and
    every parameter outside the stage's trainable set untouched, bit for bit."""
    from multishiftseg_amd import synth
    from multishiftseg_amd.deepv3 import DeepWV3Plus
    from multishiftseg_amd.loss import RelContrastiveLoss
    from multishiftseg_amd.trainer import LOSS_PARAMS, STAGE_TRAINABLE, TrainStep
    from oracle import loss as oloss
    C, pairs, h, w = 12, 2, 64, 64
    params = synth.deepwv3plus_params(112, num_classes=C)
    m = DeepWV3Plus(C)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()}, strict=True)
    m = m.cuda()
    m.uncertainty_func_init()
    step = TrainStep(m, RelContrastiveLoss(LOSS_PARAMS), stage=stage)
    step.keep_outputs = True
    assert sorted(step.names) == sorted(k for k, _ in m.named_parameters() if any(s in k for s in STAGE_TRAINABLE[stage]))
    m.dropout_masks = {k: torch.from_numpy(v) for k, v in dropout_masks(2 * pairs, seed=9).items()}
    img = torch.from_numpy(synth.synth_image(21, 2 * pairs, h, w)).cuda()
    t0 = synth.synth_targets(31, pairs, h, w, num_classes=C).astype(np.int64)
    assert t0[t0 < 99].max() < C
    n_orig, n_aug = int((t0[:pairs] < 99).sum()), int((t0[pairs:] < 99).sum())
    n_ood = int(((t0 > 99) & (t0 != 255)).sum())
    rng = np.random.default_rng(41)
    perms = [rng.permutation(k).astype(np.int64) for k in (n_orig, n_aug, n_ood)]
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    loss = step(img, torch.from_numpy(t0.copy()).cuda(), perms=[torch.from_numpy(p) for p in perms])
    score, logit = step.last_outputs
    assert tuple(logit.shape) == (2 * pairs, C, h, w)
    assert np.isfinite(loss.item())
    r = oloss.rel_contrastive_loss(logit.cpu().numpy(), score.cpu().numpy(), t0.copy(), LOSS_PARAMS, perms)
    print(f"stage {stage}: loss {loss.item():.8g}, oracle on the step's outputs {float(r['loss']):.8g}")
    np.testing.assert_allclose(loss.item(), r["loss"], rtol=1e-5)
    moved = 0
    for k, p in m.named_parameters():
        if k in step.names:
            moved += int(not torch.equal(p.detach(), before[k]))
        else:
            assert torch.equal(p.detach(), before[k]), k
    assert moved == len(step.names)              # and the trainable ones all took their Adam step


def test_evaluate(net):
    """evaluate() with an OODMeter and a SegMeter(C) on two 64 x 96 batches gives what feeding both meters by hand from the
    model's outputs gives; a SegMeter of another class count is refused before any forward. Past SegMeter's own 32 classes the
    model still evaluates the OOD half."""
    from multishiftseg_amd import synth
    from multishiftseg_amd.metric import OODMeter, SegMeter
    C, _, model = net
    batches = [(torch.from_numpy(synth.synth_image(50 + i, 2, 64, 96)).cuda(),
                torch.from_numpy(synth.synth_targets(60 + i, 1, 64, 96, num_classes=C).astype(np.int64)).cuda()) for i in range(2)]

    class Once:                                   # an iterable that records whether the sweep touched it
        def __init__(self):
            self.started = False

        def __iter__(self):
            self.started = True
            return iter(batches)
    it = Once()
    with pytest.raises(ValueError, match="19"):
        model.evaluate(it, OODMeter(), SegMeter(19))
    assert not it.started
    with_seg = C <= 32
    if with_seg:
        ood, seg = model.evaluate(batches, OODMeter(), SegMeter(C))
    else:
        with pytest.raises(ValueError):
            SegMeter(C)
        ood = model.evaluate(batches, OODMeter())
    by_hand_ood, by_hand_seg = OODMeter(), SegMeter(C) if with_seg else None
    model.eval()
    with torch.no_grad():
        for img, target in batches:
            score, logit = model(img)
            by_hand_ood.update(score, target)
            if with_seg:
                by_hand_seg.update(logit, target)
    assert ood is not None
    np.testing.assert_equal(ood, by_hand_ood.compute())
    if with_seg:
        assert seg is not None
        np.testing.assert_equal(seg, by_hand_seg.compute())
