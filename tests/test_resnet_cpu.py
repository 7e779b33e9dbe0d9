"""CPU: the ResNet-50 backbone mirror and the MaskFormer eval shell keep detectron2's / the reference's names and shapes and refuse
what is not built. No compute."""
import collections

import pytest
import torch
from torch import nn

WIDTHS = {"res2": (64, 256, 3), "res3": (128, 512, 4), "res4": (256, 1024, 6), "res5": (512, 2048, 3)}    # bottleneck, output, blocks


def expected_convs():
    """name -> weight shape, from the naming rule of detectron2's R50 (STRIDE_IN_1X1 False)."""
    convs = {"stem.conv1": (64, 3, 7, 7)}
    cin = 64
    for stage, (mid, out, nblocks) in WIDTHS.items():
        for i in range(nblocks):
            p = f"{stage}.{i}"
            if i == 0:
                convs[p + ".shortcut"] = (out, cin, 1, 1)
            convs[p + ".conv1"] = (mid, cin, 1, 1)
            convs[p + ".conv2"] = (mid, mid, 3, 3)
            convs[p + ".conv3"] = (out, mid, 1, 1)
            cin = out
    return convs


@pytest.fixture(scope="module")
def backbone():
    from multishiftseg_amd import build_resnet_backbone
    return build_resnet_backbone()


def test_state_dict_keys_and_shapes(backbone):
    sd = backbone.state_dict()
    convs = expected_convs()
    assert len(convs) == 53
    want = {}
    for name, shape in convs.items():
        want[name + ".weight"] = shape
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            want[f"{name}.norm.{leaf}"] = (shape[0],)
        want[name + ".norm.num_batches_tracked"] = ()
    assert set(sd) == set(want)
    for k, shape in want.items():
        assert tuple(sd[k].shape) == shape, k
    assert sum(1 for k, v in sd.items() if k.endswith(".weight") and v.dim() == 4) == 53
    norms = [m for m in backbone.modules() if isinstance(m, nn.BatchNorm2d)]
    assert len(norms) == 53 and all(m.eps == 1e-5 for m in norms)


def test_strides_and_paddings(backbone):
    assert (backbone.stem.conv1.stride, backbone.stem.conv1.padding, backbone.stem.conv1.bias) == ((2, 2), (3, 3), None)
    for stage in WIDTHS:
        for i, blk in enumerate(getattr(backbone, stage)):
            s = 2 if (i == 0 and stage != "res2") else 1
            assert blk.conv1.stride == (1, 1) and blk.conv3.stride == (1, 1) and blk.conv2.stride == (s, s) and blk.conv2.padding == (1, 1)
            assert (blk.shortcut is not None) == (i == 0)
            if blk.shortcut is not None:
                assert blk.shortcut.stride == (s, s)
            assert all(c.bias is None and c.dilation == (1, 1) for c in (blk.conv1, blk.conv2, blk.conv3))


def test_output_shape(backbone):
    from multishiftseg_amd import build_resnet_backbone
    shapes = backbone.output_shape()
    assert {k: (v.channels, v.stride) for k, v in shapes.items()} == {"res2": (256, 4), "res3": (512, 8), "res4": (1024, 16), "res5": (2048, 32)}
    assert list(build_resnet_backbone(out_features=("res3", "res5")).output_shape()) == ["res3", "res5"]
    assert backbone.size_divisibility == 32


def test_refusals(backbone):
    from multishiftseg_amd import build_resnet_backbone
    with pytest.raises(NotImplementedError):
        build_resnet_backbone(depth=101)
    with pytest.raises(NotImplementedError):
        build_resnet_backbone(stride_in_1x1=True)
    x = torch.zeros(1, 3, 32, 32)
    backbone.train()
    with pytest.raises(NotImplementedError, match="train-mode"):
        backbone(x)
    backbone.eval()
    with pytest.raises(NotImplementedError, match="no backward"):
        backbone(x)                                    # gradients enabled and the parameters require one
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU path"):
        backbone(x)


@pytest.mark.parametrize("metadata", [False, True])
def test_state_dict_without_counters_loads(backbone, metadata):
    """FrozenBatchNorm2d checkpoints carry no num_batches_tracked -- as a plain dict, and as a filtered state_dict() that kept the
    version metadata under which nn.BatchNorm2d reports the counter missing."""
    from multishiftseg_amd import MaskFormer, build_resnet_backbone
    full = backbone.state_dict()
    sd = collections.OrderedDict((k, v.clone()) for k, v in full.items() if not k.endswith("num_batches_tracked"))
    assert len(sd) == 53 * 5
    if metadata:
        sd._metadata = full._metadata
    fresh = build_resnet_backbone()
    res = fresh.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(fresh.res4[2].conv2.weight, backbone.res4[2].conv2.weight)
    shell = MaskFormer(build_resnet_backbone(), nn.Identity(), nn.Identity())
    nested = collections.OrderedDict(("backbone." + k, v) for k, v in sd.items())
    res = shell.load_state_dict(nested, strict=True)
    assert not res.missing_keys and not res.unexpected_keys


def test_maskformer_child_names_and_padding(backbone):
    from multishiftseg_amd import MaskFormer
    from multishiftseg_amd.m2f_trainer import build_m2f_param_groups
    from multishiftseg_amd.maskformer import padded_size
    shell = MaskFormer(backbone, nn.Linear(2, 2), nn.Linear(3, 3))
    assert [n for n, _ in shell.named_children()] == ["backbone", "sem_seg_head"]
    assert [n for n, _ in shell.sem_seg_head.named_children()] == ["pixel_decoder", "predictor"]
    keys = set(shell.state_dict())
    assert {"backbone.stem.conv1.weight", "sem_seg_head.pixel_decoder.weight", "sem_seg_head.predictor.bias"} <= keys
    groups = build_m2f_param_groups(shell, 1e-4, 0.05)
    lrs = sorted({g["lr"] for g in groups})
    assert len(lrs) == 2 and abs(lrs[0] - 1e-5) < 1e-12                     # the backbone's parameters run at 0.1 x lr
    assert (padded_size(700, 32), padded_size(1024, 32), padded_size(1, 32), padded_size(70, 0)) == (704, 1024, 32, 70)
    assert shell.size_divisibility == 32
    img = torch.arange(2 * 3 * 5 * 7, dtype=torch.float32).reshape(2, 3, 5, 7)
    pad = MaskFormer(backbone, nn.Identity(), nn.Identity(), size_divisibility=4).pad(img)
    assert pad.shape == (2, 3, 8, 8) and torch.equal(pad[..., :5, :7], img) and pad[..., 5:, :].abs().sum() == 0 and pad[..., 7:].abs().sum() == 0
    same = torch.zeros(1, 3, 64, 96)
    assert shell.pad(same) is same
