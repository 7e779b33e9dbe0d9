"""No GPU: the stock-torch restatement of loss_ood's "margin" and "bce" branches (tests/ref_ood_pixel_loss.py) against the
reference's lines transcribed with boolean indexing and against gradcheck, and the host side of the two branches in SetCriterion
and multishiftseg_amd.ood_loss: refusals and argument errors."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_ood_pixel_loss as ref
from multishiftseg_amd import HungarianMatcher, SetCriterion, class_mix_ood_loss
from multishiftseg_amd import ood_loss as OL


def transcribed(class_logits, mask_logits, ood_masks_, kind, margin):
    """criterion.py:130-161 line by line, with torch.max and the boolean-index gathers."""
    ood_mask = (ood_masks_ == 1)
    id_mask = (ood_masks_ == 0)
    class_logits = F.softmax(class_logits, dim=-1)[..., :-1]
    mask_logits = mask_logits.sigmoid()
    logits = torch.einsum("bqc,bqhw->bchw", class_logits, mask_logits)
    score = -torch.max(logits, dim=1)[0]
    score = F.interpolate(score.unsqueeze(1), size=ood_masks_.shape[-2:], mode="bilinear", align_corners=True).squeeze(1)
    ood_score = score[ood_mask]
    id_score = score[id_mask]
    if kind == "margin":
        loss = torch.pow(id_score, 2).mean()
        if ood_mask.sum() > 0:
            loss = loss + torch.pow(torch.clamp(margin - ood_score, min=0.0), 2).mean()
    else:
        loss = F.binary_cross_entropy_with_logits(id_score, torch.zeros(id_score.size(), dtype=score.dtype), reduction="mean")
        if ood_mask.sum() > 0:
            loss = loss + F.binary_cross_entropy_with_logits(ood_score, torch.ones(ood_score.size(), dtype=score.dtype), reduction="mean")
    return 0.5 * loss


def _inputs(seed, B=2, Q=5, C=3, hw=(4, 5), size=(9, 13)):
    rng = np.random.default_rng(seed)
    cls = torch.from_numpy(rng.standard_normal((B, Q, C + 1)))
    x = torch.from_numpy(rng.standard_normal((B, Q) + hw))
    ood = torch.from_numpy((rng.random((B,) + size) < 0.3).astype(np.uint8))
    return cls, x, ood


MASKS = ("mixed", "with_255", "no_ood", "no_id", "per_image")


def _mask(name, ood):
    ood = ood.clone()
    if name == "with_255":
        ood[:, :2, 3:7] = 255
        ood[1, 5, 5] = 7
    elif name == "no_ood":
        ood[ood == 1] = 0
    elif name == "no_id":
        ood[ood == 0] = 1
        ood[0, 0, 0] = 255
    elif name == "per_image":
        ood[0], ood[1] = 1, 0
    return ood


@pytest.mark.parametrize("kind,margin", [("margin", 1.0), ("margin", -0.9), ("bce", None)])
@pytest.mark.parametrize("mask", MASKS)
def test_restatement_equals_the_reference_lines_with_boolean_indexing(kind, margin, mask):
    cls, x, ood = _inputs(11)
    ood = _mask(mask, ood)
    a, b = cls.clone().requires_grad_(True), x.clone().requires_grad_(True)
    c, d = cls.clone().requires_grad_(True), x.clone().requires_grad_(True)
    got, want = ref.class_mix_ood_loss(a, b, ood, kind, margin), transcribed(c, d, ood, kind, margin)
    assert got.dim() == 0 and got.dtype == torch.float64
    if mask == "no_id":
        assert torch.isnan(got) and torch.isnan(want)              # the mean over an empty tensor
    else:
        assert torch.isfinite(want)
        np.testing.assert_allclose(float(got.detach()), float(want.detach()), rtol=1e-14)
    if kind == "margin" and margin < 0:                             # part of the OOD pixels clamp, part do not
        s = ref.score(ref.neg_max(ref.mix(cls, x)), ood.shape[-2:])[ood == 1]
        assert s.numel() == 0 or 0 < int((s < margin).sum()) < s.numel()
    got.backward()
    want.backward()
    for g, w in ((a.grad, c.grad), (b.grad, d.grad)):
        assert torch.isfinite(g).all() and (g != 0).any()           # n_id == 0: the gradients of the other term alone, not NaN
        np.testing.assert_allclose(g.numpy(), w.numpy(), rtol=1e-11, atol=1e-15)
    # any dtype of the mask, through == 1 / == 0
    for other in (ood.to(torch.float32), ood.to(torch.int64)):
        again = ref.class_mix_ood_loss(cls, x, other, kind, margin)
        assert torch.equal(torch.nan_to_num(again, nan=7.0), torch.nan_to_num(got.detach(), nan=7.0))


def test_a_pixel_in_neither_set_contributes_nothing():
    cls, x, ood = _inputs(12)
    ood[:, 2:4, :] = 255
    s = ref.score(ref.neg_max(ref.mix(cls, x)), ood.shape[-2:]).requires_grad_(True)
    for kind, margin in (("margin", 0.5), ("bce", None)):
        g, = torch.autograd.grad(ref.pixel_loss(s, ood, kind, margin), s)
        assert (g[:, 2:4, :] == 0).all() and (g[:, :2, :] != 0).all()


def test_first_max_gives_a_tie_to_the_lowest_index():
    m = torch.tensor([[[1.0], [3.0], [3.0], [2.0]]], dtype=torch.float64).unsqueeze(-1).requires_grad_(True)        # [1,4,1,1]
    t = ref.neg_max(m)
    assert float(t.detach()) == -3.0
    g, = torch.autograd.grad(t.sum(), m)
    assert g.flatten().tolist() == [0.0, -1.0, 0.0, 0.0]


@pytest.mark.parametrize("kind,margin", [("margin", 1.0), ("margin", -0.9), ("bce", None)])
def test_restatement_passes_gradcheck_in_float64(kind, margin):
    cls, x, ood = _inputs(3, B=1, Q=3, C=3, hw=(3, 2), size=(7, 5))
    ood[0, 0, :3] = 255
    assert ref.top_gap(ref.mix(cls, x)) > 1e-4                      # no tie near the point of differentiation
    if kind == "margin":                                            # and no OOD pixel on the (continuous) kink of the squared hinge
        s = ref.score(ref.neg_max(ref.mix(cls, x)), ood.shape[-2:])
        assert float((margin - s[ood == 1]).abs().min()) > 1e-4
    cls.requires_grad_(True)
    x.requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b: ref.class_mix_ood_loss(a, b, ood, kind, margin), (cls, x), eps=1e-6, atol=1e-7)


def _criterion(**kw):
    args = dict(num_classes=19, matcher=HungarianMatcher(2.0, 5.0, 5.0, num_points=8), weight_dict={}, eos_coef=0.1,
                losses=["labels", "masks", "ood"], num_points=8, oversample_ratio=3.0, importance_sample_ratio=0.75, ood_loss="margin", margin=1.0,
                deep_supervision=True)
    args.update(kw)
    return SetCriterion(**args)


def _cpu_outputs():
    z = torch.zeros
    step = lambda: {"pred_logits": z(1, 4, 20), "pred_masks": z(1, 4, 3, 3)}
    targets = [{"labels": torch.tensor([1]), "masks": z(1, 6, 6, dtype=torch.bool), "ood_mask": z(12, 12)}]
    return dict(step(), aux_outputs=[step(), step()]), targets


def test_the_host_refusal_of_margin_and_bce_comes_before_any_other_check():
    outputs, targets = _cpu_outputs()
    for mode in ("margin", "bce"):
        for kw in ({}, {"margin": None}, {"margin": float("nan")}, {"num_classes": 7}, {"losses": ["ood", "boxes"]}):
            c = _criterion(ood_loss=mode, **kw)
            with pytest.raises(NotImplementedError, match="loss_ood.*no CPU path"):
                c(outputs, targets)
            with pytest.raises(NotImplementedError, match="loss_ood.*no CPU path"):
                c.loss_ood(outputs, targets)
    for mode in (None, "rcl", "hinge", "MARGIN"):
        with pytest.raises(ValueError, match="define_ood_loss"):
            _criterion(ood_loss=mode)(outputs, targets)
    # without "ood" among the losses the two modes refuse nothing of their own: the criterion's usual CPU refusal
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):
        _criterion(losses=["labels", "masks"])(outputs, targets)


def test_argument_errors_of_the_wrappers_come_from_the_host():
    cls, x, ood = _inputs(1)
    cls, x = cls.float(), x.float()
    with pytest.raises(ValueError, match="kind"):
        class_mix_ood_loss(cls, x, ood, kind="RCL")
    for margin in (None, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="margin"):
            class_mix_ood_loss(cls, x, ood, kind="margin", margin=margin)
        with pytest.raises(ValueError, match="margin"):
            OL.ood_pixel_loss(x[:, 0], ood, "margin", margin)
    with pytest.raises(RuntimeError, match="no CPU path"):
        class_mix_ood_loss(cls, x, ood, kind="bce")
    with pytest.raises(RuntimeError, match="no CPU path"):
        OL.ood_negmax(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        OL.ood_pixel_loss(x[:, 0], ood, "bce")
    # the byte map: uint8 and bool as they are, anything else through == 1 / == 0
    assert OL.ood_mask_bytes(ood) is ood
    b = ood.bool()
    assert OL.ood_mask_bytes(b).dtype == torch.uint8 and OL.ood_mask_bytes(b).data_ptr() == b.data_ptr()
    f = torch.tensor([[[0.0, 1.0, 0.5, 255.0, -1.0, 2.0]]])
    assert OL.ood_mask_bytes(f).tolist() == [[[0, 1, 255, 255, 255, 255]]]
    assert OL.ood_mask_bytes(f.long()).tolist() == [[[0, 1, 0, 255, 255, 255]]]
    import multishiftseg_amd
    assert "class_mix_ood_loss" in multishiftseg_amd.__all__
