"""GPU: Mask2Former stage 1 through the modules -- MaskFormer.stage1_forward / semantic_inference, the predictor's `semantic`
keyword and m2f_trainer.M2FStage1Step -- on the tiny model of tests/test_gpu_maskformer_train.py (R50, one encoder layer, two
decoder layers, 8 queries, 19 classes).

The step is checked against tests/ref_stage1.py: from the frozen tensors of the model (the last decoder_norm output, pred_logits and
the low-resolution pred_masks, all read once from the device) the restatement runs class_embed2, the upsample, the mix, the crop,
1 - max_c, RelContrastiveLoss and torch.optim.Adam for three steps, in float64 and in float32. Rule of
tests/test_gpu_class_mix.py: max|hip - float64| <= 8 x floor, floor = max|float32 restatement - float64| > 0, for the three losses
(as one tensor) and for both parameters after the third step.

Conditions on the inputs (conditions, not tolerances; asserted, and checked on the restatement alone when the seeds were chosen):
in float64, at every step, the smallest gap between the two largest class maps of the ood head over all pixels is at least 64 x the
float32 floor of those maps, and no hinge argument of the loss lies within 64 x the float32 floor of the scores of its kink.
Images of 60 x 90 are padded to 64 x 96: Hp != H and Wp != W."""
import contextlib

import numpy as np
import pytest
import torch

import ref_stage1 as ref
from test_gpu_class_mix import assert_gap, held
from test_gpu_maskformer_train import C, Q, _model

pytestmark = pytest.mark.gpu
DEV = "cuda"

SIZE, PADDED = (60, 90), (64, 96)
IMAGE_SEED, TARGET_SEED = 1, 3
PAIR_SEEDS = (11, 12, 13)                                     # torch.manual_seed before each step's pairing
LR, WEIGHT_DECAY = 1e-4, 1e-4                                 # M2F.yaml:26-27
RCL = {"ce_weights": [0.5, 0.25], "conduct_pixel_selection": False, "inoutaug_contras_margins_tri": [0.7, 0.5, 0.2]}


def images(size=SIZE, seed=IMAGE_SEED):
    return torch.rand((2, 3) + tuple(size), generator=torch.Generator().manual_seed(seed))


def target(size=SIZE, seed=TARGET_SEED):
    """[orig; aug] int64: class blocks of 6 x 9 pixels, void rows in both, an OOD object (254) in the augmented image."""
    rng = np.random.default_rng(seed)
    t = np.repeat(np.repeat(rng.integers(0, C, (2, size[0] // 6 + 1, size[1] // 9 + 1)), 6, 1), 9, 2)[:, :size[0], :size[1]].astype(np.int64)
    t[:, :3, :] = 255
    t[1, 20:41, 30:61] = 254
    return torch.from_numpy(t)


def frozen(model, imgs):
    """What stage 1 never changes: (decoder_norm output of the last step [B,Q,256], pred_logits, low-resolution pred_masks NCHW)."""
    with torch.no_grad():
        feats = model.backbone(model.pad(imgs.to(DEV).float()))
        mf, _, ms = model.sem_seg_head.pixel_decoder.forward_features(feats)
        pred = model.sem_seg_head.predictor
        norms, masks, _, _ = pred._forward_frozen(ms, mf, False)
        out = pred(ms, mf, None)
    assert torch.equal(out["pred_masks"], masks[-1])
    return norms[-1].cpu(), out["pred_logits"].cpu(), masks[-1].cpu()


@contextlib.contextmanager
def restored(model):
    """Whatever a stage-1 step does to the model -- requires_grad flags, class_embed2, gradients -- undone on exit."""
    flags = {n: p.requires_grad for n, p in model.named_parameters()}
    head = model.sem_seg_head.predictor.class_embed2
    saved = {k: v.detach().clone() for k, v in head.state_dict().items()}
    try:
        yield
    finally:
        with torch.no_grad():
            for k, v in head.state_dict().items():
                v.copy_(saved[k])
        for n, p in model.named_parameters():
            p.requires_grad = flags[n]
            p.grad = None


@pytest.fixture(scope="module")
def model():
    return _model()


def _freeze_for_stage1(model):
    from multishiftseg_amd.trainer import configure_trainable_params
    return configure_trainable_params(model, ("class_embed2",))


@pytest.mark.parametrize("size", [(64, 96), SIZE])                 # unpadded; Hp != H and Wp != W
def test_stage1_forward_shapes_and_the_closed_set_prediction(model, size):
    imgs = images(size).to(DEV)
    with restored(model):
        _, names = _freeze_for_stage1(model)
        assert sorted(names) == ["sem_seg_head.predictor.class_embed2.bias", "sem_seg_head.predictor.class_embed2.weight"]
        sem, score = model.stage1_forward(imgs)
        assert tuple(sem.shape) == (2, 19) + tuple(size) and tuple(score.shape) == (2,) + tuple(size)
        assert sem.requires_grad is False and score.requires_grad
        assert bool(torch.isfinite(sem).all()) and bool(torch.isfinite(score).all())
        closed = model.semantic_inference(imgs)
        assert torch.equal(closed, sem) and not closed.requires_grad
        with torch.no_grad():
            sem0, score0 = model.stage1_forward(imgs)
        assert torch.equal(sem0, sem) and torch.equal(score0, score) and not score0.requires_grad
        # the predictor's keyword by hand: the same tensors, and the rest of its dict as without it
        with torch.no_grad():
            x = model.pad(imgs)
            feats = model.backbone(x)
            mf, _, ms = model.sem_seg_head.pixel_decoder.forward_features(feats)
            pred = model.sem_seg_head.predictor
            plain = pred(ms, mf, None)
            out = pred(ms, mf, None, semantic=(x.shape[-2], x.shape[-1]) + tuple(size))
        assert torch.equal(out["sem_seg"], sem) and torch.equal(out["ood_score"], score.detach())
        assert out["pred_masks_ood"] is out["pred_masks"]
        for k in ("pred_logits", "pred_masks", "pred_logits_ood"):
            assert torch.equal(out[k], plain[k]), k
        assert "sem_seg" not in plain and "ood_score" not in plain
        with pytest.raises(ValueError):
            pred(ms, mf, None, semantic=(64, 96, 60, 90), fuse_score=(64, 96))


def test_only_class_embed2_receives_a_gradient(model):
    imgs = images().to(DEV)
    with restored(model):
        _freeze_for_stage1(model)
        for p in model.parameters():
            p.grad = None
        sem, score = model.stage1_forward(imgs)
        score.backward(torch.randn(score.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(2)))
        got = sorted(n for n, p in model.named_parameters() if p.grad is not None)
        assert got == ["sem_seg_head.predictor.class_embed2.bias", "sem_seg_head.predictor.class_embed2.weight"]
        head = model.sem_seg_head.predictor.class_embed2
        assert bool(torch.isfinite(head.weight.grad).all()) and bool((head.weight.grad != 0).any()) and bool((head.bias.grad != 0).any())
        # a trainable parameter elsewhere in the predictor is an error, not a silently missing gradient
        model.sem_seg_head.predictor.class_embed.weight.requires_grad = True
        with pytest.raises(NotImplementedError):
            model.stage1_forward(imgs)


def restate(model, dtype):
    dn, cls, masks = frozen(model, images())
    head = model.sem_seg_head.predictor.class_embed2
    return ref.train(dn, cls, masks, head.weight, head.bias, PADDED, SIZE, target(), RCL, PAIR_SEEDS, LR, WEIGHT_DECAY, dtype)


def check_conditions(r64, r32):
    for s in range(len(PAIR_SEEDS)):
        assert_gap(f"step {s}", r64["fulls"][s], r32["fulls"][s])
        floor = float((r32["scores"][s] - r64["scores"][s]).abs().max())
        kink = float(r64["hinges"][s].abs().min())
        print(f"step {s}: smallest |hinge argument| {kink:.3e}, 64 x floor of the scores {64 * floor:.3e}")
        assert floor > 0 and kink >= 64 * floor, f"step {s}: a pair lies on the kink of its hinge: choose other seeds"
    # a loss is one float32 number, which even correctly rounded lies up to half an ulp from the float64 one (the condition of
    # tests/test_gpu_class_mix.py): the floor of the three losses, taken as one tensor, is at least 0.3 ulp of the smallest
    floor = float((r32["losses"] - r64["losses"]).abs().max())
    ulp = float(np.spacing(np.float32(r64["losses"].min())))
    print(f"losses: floor {floor:.3e} = {floor / ulp:.2f} ulp")
    assert floor >= 0.3 * ulp, "the float32 restatement happens to round the losses almost exactly: choose other seeds"


def test_three_steps_against_the_restatement_with_torch_adam(model):
    from multishiftseg_amd import M2FStage1Step
    from multishiftseg_amd.loss import RelContrastiveLoss
    with restored(model):
        r64, r32 = restate(model, torch.float64), restate(model, torch.float32)
        check_conditions(r64, r32)
        step = M2FStage1Step(model, RelContrastiveLoss(RCL, pairing="reference"), lr=LR, weight_decay=WEIGHT_DECAY)
        assert sorted(step.names) == ["sem_seg_head.predictor.class_embed2.bias", "sem_seg_head.predictor.class_embed2.weight"]
        assert [n for n, p in model.named_parameters() if p.requires_grad] == step.names
        imgs, losses = images().to(DEV), []
        for seed in PAIR_SEEDS:
            torch.manual_seed(seed)
            loss = step(imgs, target().to(DEV))
            assert loss.dim() == 0 and not loss.requires_grad
            losses.append(loss)
        head = model.sem_seg_head.predictor.class_embed2
        held("losses of the three steps", torch.stack(losses).cpu(), r64["losses"], r32["losses"])
        held("class_embed2.weight after three steps", head.weight.detach().cpu(), r64["weight"], r32["weight"])
        held("class_embed2.bias after three steps", head.bias.detach().cpu(), r64["bias"], r32["bias"])
        assert all(p.grad is None for n, p in model.named_parameters() if n not in step.names)


def test_forward_and_ood_score_do_not_change_when_a_stage1_step_is_constructed(model):
    from multishiftseg_amd import M2FStage1Step
    from multishiftseg_amd.loss import RelContrastiveLoss
    imgs = images().to(DEV)
    before, score_before = model(imgs), model.ood_score(imgs)
    with restored(model):
        M2FStage1Step(model, RelContrastiveLoss(RCL, pairing="reference"))
        after, score_after = model(imgs), model.ood_score(imgs)
    assert list(before) == list(after)
    for k in ("pred_logits", "pred_logits_ood", "ood_score"):
        assert torch.equal(before[k], after[k]), k
    for a, b in zip(before["aux_outputs"], after["aux_outputs"]):
        assert all(torch.equal(a[k], b[k]) for k in a)
    assert torch.equal(score_before, score_after) and not score_after.requires_grad
