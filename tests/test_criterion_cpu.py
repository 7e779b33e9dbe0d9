"""CPU: the stock-torch restatement of SetCriterion's losses (tests/ref_criterion.py) against torch's own functions and a case
worked by hand, its tie rule, and the host side of multishiftseg_amd.SetCriterion (no kernel runs here)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_criterion as ref
from multishiftseg_amd import HungarianMatcher, SetCriterion
from multishiftseg_amd import kernels as K
from multishiftseg_amd.criterion import selection_counts


def test_restatement_agrees_with_the_stock_torch_functions():
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(37, 6, generator=g, dtype=torch.float64) * 3
    tc = torch.randint(0, 6, (37,), generator=g)
    w = torch.ones(6, dtype=torch.float64)
    w[-1] = 0.1
    assert torch.allclose(ref.label_loss(logits, tc, w), F.cross_entropy(logits, tc, w), rtol=1e-13, atol=0)
    x = torch.randn(5, 33, generator=g, dtype=torch.float64) * 20
    t = torch.rand(5, 33, generator=g, dtype=torch.float64)
    assert torch.allclose(ref.bce_with_logits(x, t), F.binary_cross_entropy_with_logits(x, t, reduction="none"), rtol=1e-13, atol=1e-15)
    s = x.sigmoid()
    dice = 1 - (2 * (s * t).sum(-1) + 1) / (s.sum(-1) + t.sum(-1) + 1)          # dice_loss of the reference, before / num_masks
    assert torch.allclose(ref.dice_terms(x, t), dice, rtol=1e-13, atol=0)
    # mask_losses = the two formulas on the sampled maps
    src = torch.randn(3, 5, 4, generator=g, dtype=torch.float64)
    tgt = (torch.rand(3, 9, 4, generator=g) < 0.5).to(torch.float64)
    pts = torch.rand(3, 17, 2, generator=g, dtype=torch.float64)
    xs = torch.stack([ref.point_sample(src[r][None], pts[r])[0] for r in range(3)])
    ts = torch.stack([ref.point_sample(tgt[r][None], pts[r])[0] for r in range(3)])
    lm, ld = ref.mask_losses(src, tgt, pts, 7.0)
    assert torch.allclose(lm, F.binary_cross_entropy_with_logits(xs, ts, reduction="none").mean(1).sum() / 7.0, rtol=1e-13, atol=0)
    assert torch.allclose(ld, ref.dice_terms(xs, ts).sum() / 7.0, rtol=1e-13, atol=0)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_restatement_differentiates_the_mask_loss_at_zero_logits(dtype):
    """The yardstick of the gradients is autograd of the restatement: at x == +-0.0 (an all-zero source map) it must give
    sigmoid(0) - t = 1/2 - t, not a one-sided slope of a clamp or an abs; and F.binary_cross_entropy_with_logits' gradient elsewhere."""
    x = torch.tensor([0.0, -0.0, 0.0, 3.0, -3.0, 80.0, -80.0], dtype=dtype, requires_grad=True)
    t = torch.tensor([0.0, 1.0, 0.25, 0.5, 0.5, 1.0, 0.0], dtype=dtype)
    ref.bce_with_logits(x, t).sum().backward()
    assert x.grad[:3].tolist() == [0.5, -0.5, 0.25]
    y = x.detach().clone().requires_grad_(True)
    F.binary_cross_entropy_with_logits(y, t, reduction="sum").backward()
    assert torch.allclose(x.grad, y.grad, rtol=4 * torch.finfo(dtype).eps, atol=0)
    src = torch.zeros((1, 2, 3), dtype=dtype, requires_grad=True)               # through mask_losses: one point at a pixel centre
    lm, _ = ref.mask_losses(src, torch.ones((1, 2, 3), dtype=dtype), torch.tensor([[[0.5, 0.25]]], dtype=dtype), 1.0)
    lm.backward()
    assert src.grad[0, 0, 1] == -0.5 and float(src.grad.abs().sum()) == 0.5


def test_two_points_one_row_by_hand():
    """A 1x1 source map of value 2 and a 1x1 target of 1: at the centre both samples are the pixel, at (0, 0) a quarter of it."""
    src = torch.full((1, 1, 1), 2.0, dtype=torch.float64)
    tgt = torch.ones((1, 1, 1), dtype=torch.float64)
    pts = torch.tensor([[[0.5, 0.5], [0.0, 0.0]]], dtype=torch.float64)
    x, t = (2.0, 0.5), (1.0, 0.25)
    sg = [1 / (1 + math.exp(-v)) for v in x]
    bce = [max(v, 0) - v * u + math.log1p(math.exp(-abs(v))) for v, u in zip(x, t)]
    want_mask = (bce[0] + bce[1]) / 2 / 3.0
    want_dice = (1 - (2 * (sg[0] * t[0] + sg[1] * t[1]) + 1) / (sg[0] + sg[1] + t[0] + t[1] + 1)) / 3.0
    lm, ld = ref.mask_losses(src, tgt, pts, 3.0)
    assert abs(float(lm) - want_mask) < 1e-15 and abs(float(ld) - want_dice) < 1e-15
    outputs = [{"pred_logits": torch.tensor([[[1.0, 3.0]]], dtype=torch.float64), "pred_masks": src[None]}]
    targets = [{"labels": torch.tensor([0]), "masks": tgt}]
    got = ref.criterion(outputs, targets, [[[0]]], pts, num_classes=1, eos_coef=0.1, num_masks=3.0)
    assert list(got) == ["loss_ce", "loss_mask", "loss_dice"]
    assert abs(float(got["loss_ce"]) - (math.log(math.exp(1) + math.exp(3)) - 1)) < 1e-14
    assert abs(float(got["loss_mask"]) - want_mask) < 1e-15


@pytest.mark.parametrize("mode", ["uncertain", "clean"])
def test_ties_go_to_the_lowest_candidate_index(mode):
    g = torch.Generator().manual_seed(1)
    cand = torch.rand(195, 2, generator=g)
    tgt = torch.zeros(9, 4)
    for src in (torch.zeros(5, 3), torch.where(torch.rand(5, 3, generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))):
        for dtype in (torch.float64, torch.float32):
            assert ref.select_points(src, tgt, cand, 48, mode, dtype).tolist() == list(range(48))
    src = torch.randn(5, 3, generator=g)
    src[2, 1] = float("nan")                                    # a NaN key ranks below every number
    idx = ref.select_points(src, tgt, cand, 150, "uncertain")
    keys = ref.selection_keys(src, tgt, cand, "uncertain")
    n_num = int((~keys.isnan()).sum())
    assert n_num < 150 and set(torch.nonzero(~keys.isnan())[:, 0].tolist()) <= set(idx.tolist())
    assert [i for i in idx.tolist() if math.isnan(float(keys[i]))] == torch.nonzero(keys.isnan())[:150 - n_num, 0].tolist()
    rnd = torch.randn(5, 3, generator=g)
    idx = ref.select_points(rnd, tgt, cand, 48, "uncertain").tolist()
    keys = ref.selection_keys(rnd, tgt, cand, "uncertain")
    assert idx == sorted(idx) and len(set(idx)) == 48 and float(keys[idx].min()) >= float(np.delete(keys.numpy(), idx).max())


def _criterion(**kw):
    args = dict(num_classes=19, matcher=HungarianMatcher(2.0, 5.0, 5.0, num_points=12544), weight_dict={"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0},
                eos_coef=0.1, losses=["labels", "masks"], num_points=12544, oversample_ratio=3.0, importance_sample_ratio=0.75,
                ood_loss="RCL", margin=1.0, deep_supervision=True)
    args.update(kw)
    return SetCriterion(**args)


def test_construction_repr_and_buffer():
    c = _criterion()
    assert c.empty_weight.shape == (20,) and c.empty_weight[:-1].eq(1).all() and float(c.empty_weight[-1]) == pytest.approx(0.1)
    assert "empty_weight" in dict(c.named_buffers()) and c.extra_loss is None and c.mask_loss_with_pixel_selection is False
    c.set_extra_loss("x")
    assert c.extra_loss == "x"
    lines = repr(c).split("\n")
    assert lines[0] == "Criterion SetCriterion" and lines[1] == "    matcher: Matcher HungarianMatcher"
    assert lines[2:5] == ["        cost_class: 2.0", "        cost_mask: 5.0", "        cost_dice: 5.0"]
    assert lines[5:] == ["    losses: ['labels', 'masks']", "    weight_dict: {'loss_ce': 2.0, 'loss_mask': 5.0, 'loss_dice': 5.0}", "    num_classes: 19",
                         "    eos_coef: 0.1", "    num_points: 12544", "    oversample_ratio: 3.0", "    importance_sample_ratio: 0.75"]
    positional = SetCriterion(19, c.matcher, {}, 0.1, ["labels"], 112, 3.0, 0.75, "RCL", 1.0, False)       # the reference's argument order
    assert positional.num_points == 112 and positional.ood_loss == "RCL" and positional.margin == 1.0 and positional.deep_supervision is False


def test_selection_counts_of_the_shipped_config():
    assert selection_counts(12544, 3.0, 0.75) == (37632, 9408)
    assert _criterion().selection() == ("uncertain", 37632, 9408)
    assert _criterion(mask_loss_with_pixel_selection=True).selection() == ("clean", 15680, 11916)
    assert (int(12544 * ref.CLEAN_K), int(ref.CLEAN_KEEP * 12544)) == (15680, 11916)


def test_ood_and_cpu_tensors_fail_loudly():
    outputs = {"pred_logits": torch.zeros(1, 4, 20), "pred_masks": torch.zeros(1, 4, 3, 3)}
    targets = [{"labels": torch.tensor([1]), "masks": torch.zeros(1, 6, 6, dtype=torch.bool)}]
    with pytest.raises(NotImplementedError, match="loss_ood"):
        _criterion(losses=["labels", "masks", "ood"])(outputs, targets)
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):
        _criterion()(outputs, targets)
    z = torch.zeros
    i32 = dict(dtype=torch.int32)
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):
        K.m2f_point_select([z(1, 4, 3, 3)], z(1, 6, 6, dtype=torch.uint8), z(2, **i32), z(1, 1, 1, **i32), z(1, 1, 6, 2), z(1, 2, 2), 2, 4)
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):
        K.m2f_mask_loss([z(1, 4, 3, 3)], z(1, 6, 6, dtype=torch.uint8), z(2, **i32), z(1, 1, 1, **i32), z(1, 4, 2))
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):
        K.m2f_label_loss([z(1, 4, 20)], z(1, **i32), z(2, **i32), z(1, 1, 1, **i32), z(20), None, 4, (1.0,))
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):
        K.m2f_mask_loss_backward([z(1, 4, 3, 3)], z(1, 6, 6, dtype=torch.uint8), z(2, **i32), z(1, 1, 1, **i32), z(1, **i32), z(1, 4, 2),
                                 z(1, 4, dtype=torch.float64), z(1, 3), (1.0,))
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):
        K.m2f_label_loss_backward([z(1, 4, 20)], z(1, 1, 4, **i32), z(1, **i32), z(20), z(1, dtype=torch.float64), z(1, 3))
