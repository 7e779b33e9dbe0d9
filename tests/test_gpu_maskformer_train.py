"""GPU: a whole-model stage-2 step through MaskFormer.set_trainable(): backbone (res2..res5 convolution weights, the faithful
freezing pattern of ResNet.freeze) -> pixel decoder -> GMA predictor -> SetCriterion -> clipped AdamW. Smallest full configuration
(the one of tests/test_gpu_maskformer_eval.py): the R50, one encoder layer, two decoder layers, 8 queries, 19 classes, one
2 x 3 x 64 x 96 batch with synthetic targets.

Chain check: d loss / d features taken with torch.autograd.grad at the pixel decoder's inputs, pushed through the float64 restatement
of the backbone (tests/ref_resnet_grad.py); the backbone gradients of the whole backward meet the bound of
tests/test_gpu_resnet_backward.py under the same gate-pattern condition."""
import numpy as np
import pytest
import torch

import ref_resnet as RR
import ref_resnet_grad as RG
import ref_transformer_decoder as RT
from test_gpu_resnet_backward import BACKBONE_FACTOR, NAMES, _check_all, _same_pattern

pytestmark = pytest.mark.gpu

DEV = "cuda"
Q, LAYERS, C = 8, 2, 19
IMAGE_SEED = 1                     # with backbone seed 7: same ReLU patterns in float32 and float64 (checked on the CPU)
BASE_LR = 1e-4


def _model():
    from multishiftseg_amd import MaskFormer, MultiScaleMaskedTransformerDecoder_GMA, build_resnet_backbone
    from multishiftseg_amd.msdeformattn_decoder import MSDeformAttnPixelDecoder
    torch.manual_seed(3)
    backbone = RR.randomize_(build_resnet_backbone(), 7)
    decoder = MSDeformAttnPixelDecoder(backbone.output_shape(), transformer_dropout=0.0, transformer_nheads=8, transformer_dim_feedforward=128,
                                       transformer_enc_layers=1, conv_dim=256, mask_dim=256, norm="GN",
                                       transformer_in_features=["res3", "res4", "res5"], common_stride=4)
    predictor = MultiScaleMaskedTransformerDecoder_GMA(256, True, num_classes=C, hidden_dim=256, num_queries=Q, nheads=8, dim_feedforward=128,
                                                       dec_layers=LAYERS, pre_norm=False, mask_dim=256, enforce_input_project=False)
    predictor.load_state_dict(RT.synth_state_dict(41, num_layers=LAYERS, num_queries=Q, dim_feedforward=128), strict=True)
    m = MaskFormer(backbone, decoder, predictor).cuda().eval()
    m.backbone.freeze(1, norms=True)
    return m


def _criterion():
    from multishiftseg_amd import HungarianMatcher, SetCriterion, m2f_weight_dict
    weight_dict = m2f_weight_dict(2.0, 5.0, 5.0, 1.0, LAYERS + 1, True)
    return SetCriterion(C, HungarianMatcher(2.0, 5.0, 5.0, num_points=33), weight_dict, 0.1, ["labels", "masks"], 65, 3.0, 0.75, None, None,
                        True).to(DEV)


def _batch():
    images = torch.rand((2, 3, 64, 96), generator=torch.Generator().manual_seed(IMAGE_SEED))
    rng = np.random.default_rng(5)
    targets = [{"labels": torch.tensor([3, 7 + b], device=DEV), "masks": torch.from_numpy(rng.random((2, 16, 24)) < 0.5).to(DEV)}
               for b in range(2)]
    return images, targets


@pytest.fixture(scope="module")
def model():
    return _model()


def test_off_the_shell_is_the_evaluation_shell(model):
    """Without set_trainable() -- and with it, under no_grad -- ood_score is the parent's: the frozen composition of the parts."""
    images, _ = _batch()
    images = images.cuda()
    assert model._trainable is False and any(p.requires_grad for p in model.backbone.parameters())
    want = model.ood_score(images)                   # grad mode enabled, trainable parameters: still the no_grad evaluation path
    with torch.no_grad():
        feats = model.backbone(model.pad(images))
        mf, _, ms = model.sem_seg_head.pixel_decoder.forward_features(feats)
        hand = model.sem_seg_head.predictor(ms, mf, None, fuse_score=(64, 96, 64, 96))["ood_score"]
    assert torch.equal(want, hand) and not want.requires_grad
    model.set_trainable()
    try:
        with torch.no_grad():
            assert torch.equal(model.ood_score(images), want)
    finally:
        model.set_trainable(False)
    assert model.backbone._trainable is False and model.sem_seg_head.predictor._trainable is False


def test_backbone_gradients_of_the_whole_backward_are_the_chain_rule(model):
    from multishiftseg_amd import weighted_losses
    images, targets = _batch()
    crit = _criterion()
    model.set_trainable()
    try:
        for p in model.parameters():
            p.grad = None
        torch.manual_seed(5)
        x = model.pad(images.cuda())
        feats = model.backbone(x)
        mask_features, _, multi_scale = model.sem_seg_head.pixel_decoder.forward_features(feats)
        out = model.sem_seg_head.predictor(multi_scale, mask_features, None)
        total = sum(weighted_losses(crit(out, targets), crit.weight_dict).values())
        named = [(n, p) for n, p in model.backbone.named_parameters() if p.requires_grad]
        # ONE backward pass (the nodes free what they stored as it passes): the features' gradients and the backbone's together
        both = torch.autograd.grad(total, [feats[n] for n in NAMES] + [p for _, p in named])
        gfeat, gparam = both[:len(NAMES)], both[len(NAMES):]
    finally:
        model.set_trainable(False)
    gm = {n: g.detach().cpu() for n, g in zip(NAMES, gfeat)}
    assert all(float(g.abs().max()) > 0 for g in gm.values())
    sd = {k: v.cpu() for k, v in model.backbone.state_dict().items()}
    o64, g64, t64 = RG.resnet50_grads(x.cpu(), sd, gm, torch.float64)
    _, g32, t32 = RG.resnet50_grads(x.cpu(), sd, gm, torch.float32)
    flips = RG.same_gates(t32, t64)
    assert flips == 0, f"{flips} ReLU inputs change sign between float32 and float64 on the CPU: choose another seed"
    for n in NAMES:
        _same_pattern(n, feats[n].detach(), o64[n])
    got = {n: g for (n, _), g in zip(named, gparam)}
    assert len(got) == 52 and all(".norm." not in n and not n.startswith("stem.") for n in got)
    _check_all("whole step", got, {n: g64[n] for n in got}, g32, BACKBONE_FACTOR)


def test_one_train_step_moves_the_backbone_at_a_tenth_of_the_rate(model):
    from multishiftseg_amd import M2FTrainStep, build_m2f_optimizer
    images, targets = _batch()
    crit = _criterion()
    model.set_trainable()
    try:
        opt = build_m2f_optimizer(model, base_lr=BASE_LR, weight_decay=0.05, clip_value=0.01)
        rate = {id(g["params"][0]): g["lr"] for g in opt.param_groups}
        before = {n: p.detach().clone() for n, p in model.named_parameters()}
        torch.manual_seed(5)
        losses, norm = M2FTrainStep(model, crit, opt)(images.cuda(), targets=targets)
    finally:
        model.set_trainable(False)
    assert losses and all(bool(torch.isfinite(v)) for v in losses.values()), losses
    assert bool(torch.isfinite(norm)) and float(norm) > 0
    trainable = [(n, p) for n, p in model.backbone.named_parameters() if p.requires_grad]
    assert len(trainable) == 52
    for n, p in trainable:
        assert rate[id(p)] == pytest.approx(0.1 * BASE_LR), n
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
        assert not torch.equal(p.detach(), before["backbone." + n]) and bool(torch.isfinite(p).all()), n
    for n, p in model.backbone.named_parameters():
        if not p.requires_grad:
            assert id(p) not in rate and torch.equal(p.detach(), before["backbone." + n]), n
    head = [g["lr"] for g in opt.param_groups if id(g["params"][0]) not in {id(p) for _, p in trainable}]
    assert head and all(lr == pytest.approx(BASE_LR) for lr in head)
    moved = [n for n, p in model.sem_seg_head.named_parameters() if not torch.equal(p.detach(), before["sem_seg_head." + n])]
    assert any(n.startswith("pixel_decoder.") for n in moved) and any(n.startswith("predictor.") for n in moved)
