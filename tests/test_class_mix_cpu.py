"""No GPU: the stock-torch restatement of the class mix (tests/ref_class_mix.py) against a hand-worked case and gradcheck, and the
host side of SetCriterion.loss_ood: key order, refusals, CPU tensors."""
import numpy as np
import pytest
import torch

import ref_class_mix as ref
from multishiftseg_amd import HungarianMatcher, SetCriterion, class_mix_upsample
from multishiftseg_amd import kernels as K


def _sigmoid(v):
    return 1.0 / (1.0 + np.exp(-v))


def test_restatement_equals_a_hand_worked_case():
    """1 query, 2 classes, 2 x 2 -> 4 x 4: P = softmax(cls)[:2], M[c] = P[c] sigmoid(x); per axis the four outputs are
    v0, 0.75 v0 + 0.25 v1, 0.25 v0 + 0.75 v1, v1 (source coordinates max(0, (o + 0.5) / 2 - 0.5) = 0, 0.25, 0.75, 1.25)."""
    cls = np.array([[[1.0, -0.5, 0.25]]])
    x = np.array([[[[0.3, -1.2], [2.0, 0.0]]]])
    e = np.exp(cls[0, 0])
    P = e[:2] / e.sum()
    M = P[:, None, None] * _sigmoid(x[0, 0])[None]
    A = np.array([[1, 0], [0.75, 0.25], [0.25, 0.75], [0, 1]])
    full = np.einsum("ya,cab,xb->cyx", A, M, A)
    tc, tx = torch.from_numpy(cls), torch.from_numpy(x)
    m, p = ref.mix(tc, tx)
    np.testing.assert_allclose(p.numpy()[0, 0], P, rtol=1e-14)
    np.testing.assert_allclose(m.numpy()[0], M, rtol=1e-14)
    np.testing.assert_allclose(ref.class_mix_upsample(tc, tx, (4, 4), (4, 4), "logits").numpy()[0], full, rtol=1e-13)
    np.testing.assert_allclose(ref.class_mix_upsample(tc, tx, (4, 4), (3, 2), "neg_max").numpy()[0], -full.max(0)[:3, :2], rtol=1e-13)


def test_the_crop_keeps_the_scale_of_the_full_size():
    """8 -> 32 cropped to 29: output pixel o reads source max(0, (o + 0.5) * 8 / 32 - 0.5), not (o + 0.5) * 8 / 29 - 0.5."""
    rng = np.random.default_rng(0)
    m = torch.from_numpy(rng.standard_normal((1, 2, 8, 8)))
    got = ref.upsample(m, (32, 32), (29, 30), "logits")
    assert tuple(got.shape) == (1, 2, 29, 30)
    for oy, ox in ((0, 0), (7, 13), (28, 29), (17, 2)):
        sy, sx = max(0.0, (oy + 0.5) * 8 / 32 - 0.5), max(0.0, (ox + 0.5) * 8 / 32 - 0.5)
        y0, x0 = int(sy), int(sx)
        y1, x1 = min(y0 + 1, 7), min(x0 + 1, 7)
        ly, lx = sy - y0, sx - x0
        v = m[0, :, [y0, y0, y1, y1], [x0, x1, x0, x1]].numpy()
        want = (1 - ly) * ((1 - lx) * v[:, 0] + lx * v[:, 1]) + ly * ((1 - lx) * v[:, 2] + lx * v[:, 3])
        np.testing.assert_allclose(got[0, :, oy, ox].numpy(), want, rtol=1e-13)
    other = torch.nn.functional.interpolate(m, size=(29, 30), mode="bilinear", align_corners=False)
    assert float((other - got).abs().max()) > 1e-3


def test_first_max_gives_a_tie_to_the_lowest_index():
    v = torch.tensor([[[1.0], [3.0], [3.0], [2.0]]], dtype=torch.float64).unsqueeze(-1).requires_grad_(True)      # [1,4,1,1]
    out = ref.first_max(v)
    assert float(out.detach()) == 3.0
    g, = torch.autograd.grad(out.sum(), v)
    assert g.flatten().tolist() == [0.0, 1.0, 0.0, 0.0]


@pytest.mark.parametrize("mode", ["logits", "neg_max"])
def test_restatement_passes_gradcheck_in_float64(mode):
    rng = np.random.default_rng(3)
    cls = torch.from_numpy(rng.standard_normal((1, 3, 4))).requires_grad_(True)
    x = torch.from_numpy(rng.standard_normal((1, 3, 3, 2))).requires_grad_(True)
    full = ref.bilinear(ref.mix(cls, x)[0].detach(), (7, 5), (6, 5))
    assert ref.top_gap(full) > 1e-4                                 # no tie near the point of differentiation
    assert torch.autograd.gradcheck(lambda a, b: ref.class_mix_upsample(a, b, (7, 5), (6, 5), mode), (cls, x), eps=1e-6, atol=1e-7)


def _criterion(**kw):
    args = dict(num_classes=19, matcher=HungarianMatcher(2.0, 5.0, 5.0, num_points=8), weight_dict={}, eos_coef=0.1,
                losses=["labels", "masks", "ood"], num_points=8, oversample_ratio=3.0, importance_sample_ratio=0.75, ood_loss="RCL", margin=1.0,
                deep_supervision=True)
    args.update(kw)
    return SetCriterion(**args)


def _cpu_outputs():
    z = torch.zeros
    step = lambda: {"pred_logits": z(1, 4, 20), "pred_masks": z(1, 4, 3, 3), "pred_logits_ood": z(1, 4, 20), "pred_masks_ood": z(1, 4, 3, 3)}
    targets = [{"labels": torch.tensor([1]), "masks": z(1, 6, 6, dtype=torch.bool), "ood_mask": z(12, 12), "sem_seg": np.zeros((11, 10), np.int64)}]
    return dict(step(), aux_outputs=[step(), step()]), targets


def test_refusals_of_the_host_side():
    outputs, targets = _cpu_outputs()
    for mode in ("margin", "bce"):
        c = _criterion(ood_loss=mode)
        c.set_extra_loss(lambda a, b, t: a.sum())
        with pytest.raises(NotImplementedError, match="loss_ood"):
            c(outputs, targets)
        with pytest.raises(NotImplementedError, match="loss_ood"):
            c.loss_ood(outputs, targets)
    with pytest.raises(NotImplementedError, match="loss_ood"):
        _criterion()(outputs, targets)                              # RCL without an extra_loss: before anything else
    for mode in (None, "rcl", "hinge"):
        c = _criterion(ood_loss=mode)
        c.set_extra_loss(lambda a, b, t: a.sum())
        with pytest.raises(ValueError, match="define_ood_loss"):
            c(outputs, targets)
    c = _criterion()
    c.set_extra_loss(lambda a, b, t: a.sum())
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):
        c(outputs, targets)
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):
        c.loss_ood(outputs, targets)
    with pytest.raises(ValueError, match="mode"):
        class_mix_upsample(outputs["pred_logits"], outputs["pred_masks"], (12, 12), (11, 10), "max")


def test_key_order_with_ood_and_deep_supervision(monkeypatch):
    """Per step, the losses in the order of self.losses (criterion.py:455-467); the device work is replaced by stand-ins."""
    import multishiftseg_amd.criterion as crit_mod
    outputs, targets = _cpu_outputs()

    class Table:
        @staticmethod
        def apply(plan, *tensors):
            return torch.zeros(plan.S, 3)
    monkeypatch.setattr(crit_mod, "_CriterionFunction", Table)
    monkeypatch.setattr(crit_mod.K, "m2f_point_select", lambda *a, **k: None)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    for losses, per_step in ((["labels", "masks", "ood"], ["loss_ce", "loss_mask", "loss_dice", "loss_ood"]),
                             (["ood", "masks", "labels"], ["loss_ood", "loss_mask", "loss_dice", "loss_ce"]),
                             (["ood"], ["loss_ood"])):
        c = _criterion(losses=losses)
        c.set_extra_loss(lambda a, b, t: a)
        monkeypatch.setattr(c.matcher, "_pack_targets", lambda targets, dev: (None, None, None, [1]))
        monkeypatch.setattr(c.matcher, "match_steps", lambda *a, **k: None)
        monkeypatch.setattr(c, "loss_ood", lambda outputs, targets: {"loss_ood": torch.zeros(())})
        got = list(c(outputs, targets, point_candidates=torch.zeros(1), random_points=torch.zeros(1)))
        assert got == per_step + [f"{k}_{i}" for i in range(2) for k in per_step]
        c.deep_supervision = False
        assert list(c(outputs, targets, point_candidates=torch.zeros(1), random_points=torch.zeros(1))) == per_step


def test_the_new_wrappers_refuse_cpu_tensors():
    z = torch.zeros
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):
        K.m2f_class_mix(z(1, 4, 20), z(1, 4, 3, 3))
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):
        K.m2f_mix_upsample(z(1, 19, 3, 3), (12, 12), (11, 10), "logits")
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):
        K.m2f_mix_upsample_backward(z(1, 19, 3, 3), (12, 12), (11, 10), dscore=z(1, 11, 10))
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):
        K.m2f_class_mix_backward(z(1, 19, 3, 3), z(1, 4, 19), z(1, 4, 20), z(1, 4, 3, 3))
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):
        class_mix_upsample(z(1, 4, 20), z(1, 4, 3, 3), (12, 12), (11, 10), "neg_max")
