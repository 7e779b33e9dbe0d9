"""GPU: the MaskFormer eval shell (multishiftseg_amd/maskformer.py) adds no arithmetic: ood_score is, bit for bit, the composition of
its parts done by hand, and evaluate() is OODMeter over the same maps. Smallest full configuration: the R50, a pixel decoder with
one encoder layer, a predictor with two decoder layers, 8 queries and 19 classes."""
import pytest
import torch

import ref_resnet as RR
import ref_transformer_decoder as RT

pytestmark = pytest.mark.gpu

Q, LAYERS = 8, 2


@pytest.fixture(scope="module")
def shell():
    from multishiftseg_amd import MaskFormer, MultiScaleMaskedTransformerDecoder_GMA, build_resnet_backbone
    from multishiftseg_amd.msdeformattn_decoder import MSDeformAttnPixelDecoder
    torch.manual_seed(3)
    backbone = RR.randomize_(build_resnet_backbone(), 7)
    decoder = MSDeformAttnPixelDecoder(backbone.output_shape(), transformer_dropout=0.0, transformer_nheads=8, transformer_dim_feedforward=128,
                                       transformer_enc_layers=1, conv_dim=256, mask_dim=256, norm="GN",
                                       transformer_in_features=["res3", "res4", "res5"], common_stride=4)
    predictor = MultiScaleMaskedTransformerDecoder_GMA(256, True, num_classes=19, hidden_dim=256, num_queries=Q, nheads=8, dim_feedforward=128,
                                                       dec_layers=LAYERS, pre_norm=False, mask_dim=256, enforce_input_project=False)
    predictor.load_state_dict(RT.synth_state_dict(41, num_layers=LAYERS, num_queries=Q, dim_feedforward=128), strict=True)
    m = MaskFormer(backbone, decoder, predictor).cuda().eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def by_hand(shell, images, pad_to):
    H, W = images.shape[-2:]
    x = images.new_zeros(images.shape[:2] + pad_to)
    x[..., :H, :W] = images
    with torch.no_grad():
        feats = shell.backbone(x)
        mask_features, _, multi_scale = shell.sem_seg_head.pixel_decoder.forward_features(feats)
        return shell.sem_seg_head.predictor(multi_scale, mask_features, None, fuse_score=pad_to + (H, W))["ood_score"]


def test_ood_score_is_the_composition_of_the_parts(shell):
    images = torch.rand((2, 3, 70, 100), generator=torch.Generator().manual_seed(1)).cuda()
    score = shell.ood_score(images)
    assert score.shape == (2, 70, 100) and score.dtype == torch.float32 and bool(torch.isfinite(score).all())
    assert torch.equal(score, by_hand(shell, images, (96, 128)))
    out = shell(images)
    assert torch.equal(out["ood_score"], score) and out["pred_logits"].shape == (2, Q, 20)
    assert float(score.std()) > 0                                     # a map, not a constant


def test_image_already_divisible_takes_the_same_path_with_or_without_padding(shell):
    from multishiftseg_amd import MaskFormer
    images = torch.rand((1, 3, 64, 96), generator=torch.Generator().manual_seed(2)).cuda()
    score = shell.ood_score(images)
    unpadded = MaskFormer(shell.backbone, shell.sem_seg_head.pixel_decoder, shell.sem_seg_head.predictor, size_divisibility=0).eval()
    assert score.shape == (1, 64, 96)
    assert torch.equal(score, unpadded.ood_score(images))
    assert torch.equal(score, by_hand(shell, images, (64, 96)))


def test_evaluate_is_the_meter_over_the_same_maps(shell):
    from multishiftseg_amd.metric import OODMeter
    g = torch.Generator().manual_seed(4)
    batches = []
    for _ in range(3):
        images = torch.rand((2, 3, 70, 100), generator=g).cuda()
        target = torch.randint(0, 2, (2, 70, 100), generator=g).cuda()
        batches.append((images, target))
    got = shell.evaluate(batches)
    meter = OODMeter()
    meter.update(torch.cat([shell.ood_score(i) for i, _ in batches]), torch.cat([t for _, t in batches]))
    want = meter.compute()
    assert got is not None and got == want
    assert shell.evaluate(batches, meter=OODMeter()) == want
