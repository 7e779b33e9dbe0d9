"""GPU: the ResNet-50 backbone (multishiftseg_amd/resnet.py) against the stock-torch restatement (tests/ref_resnet.py) in float64.

Yardstick: for each returned map e = max|out - ref64| / max|ref64|; e_hip is ours, e_t32 the same restatement run in float32 with
stock torch on the CPU. Asserted: e_hip <= 4 * e_t32 -- both are fp32 accumulations of the same lengths; the factor covers a
different summation order and the folded norm's one extra rounding per layer. The yardstick is never our own output."""
import pytest
import torch

import ref_resnet as R

pytestmark = pytest.mark.gpu

SIZES = [(2, 3, 64, 96), (1, 3, 70, 100)]          # the second is no multiple of 32: every stride-2 layer sees an odd size
NAMES = ("res2", "res3", "res4", "res5")


@pytest.fixture(scope="module")
def model():
    from multishiftseg_amd import build_resnet_backbone
    m = R.randomize_(build_resnet_backbone(), 7).eval()
    for p in m.parameters():
        p.requires_grad_(False)
    return m.cuda()


@pytest.fixture(scope="module")
def refs(model):
    """Per size: the image, the float64 maps and the float32 stock-torch maps' errors, computed once on the CPU."""
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    out = {}
    for size in SIZES:
        img = torch.randn(size, generator=torch.Generator().manual_seed(size[2]))
        with torch.no_grad():
            r64 = R.resnet50(img.double(), R.cast(sd, torch.float64))
            r32 = R.resnet50(img, R.cast(sd, torch.float32))
        out[size] = (img, r64, {n: R.rel_max_err(r32[n], r64[n]) for n in NAMES})
    return out


@pytest.mark.parametrize("size", SIZES)
def test_backbone_within_four_times_stock_float32(model, refs, size):
    img, r64, e_t32 = refs[size]
    got = model(img.cuda())
    assert list(got) == list(NAMES)
    for n in NAMES:
        assert got[n].shape == r64[n].shape and got[n].dtype == torch.float32 and got[n].is_contiguous()
        e_hip = R.rel_max_err(got[n], r64[n])
        print(f"resnet50 {size} {n}: e_hip {e_hip:.3e}  e_t32 {e_t32[n]:.3e}  ratio {e_hip / e_t32[n]:.2f}")
        assert e_hip <= 4 * e_t32[n], (n, e_hip, e_t32[n])


@pytest.mark.parametrize("kind", ["shortcut_stride2", "shortcut_stride1", "identity"])
def test_one_block_alone(kind):
    """Block edges at 2 x 64 x 9 x 13 (odd sizes under the stride): with a shortcut and stride 2, with a shortcut and stride 1
    (res2.0's shape), and without a shortcut."""
    from multishiftseg_amd import kernels as K
    from multishiftseg_amd.resnet import BottleneckBlock
    cout, mid, stride = {"shortcut_stride2": (256, 64, 2), "shortcut_stride1": (256, 64, 1), "identity": (64, 16, 1)}[kind]
    blk = R.randomize_(BottleneckBlock(64, cout, bottleneck_channels=mid, stride=stride), 3, conv3_scale=1.0).eval().cuda()
    assert (blk.shortcut is None) == (kind == "identity")
    sd = {"b." + k: v.cpu() for k, v in blk.state_dict().items()}
    x = torch.randn((2, 64, 9, 13), generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        r64 = R.block(x.double(), R.cast(sd, torch.float64), "b", stride)
        r32 = R.block(x, R.cast(sd, torch.float32), "b", stride)
        got = blk.forward_act(K.nchw_to_act(x.cuda())).nchw()
    e_hip, e_t32 = R.rel_max_err(got, r64), R.rel_max_err(r32, r64)
    print(f"block {kind}: e_hip {e_hip:.3e}  e_t32 {e_t32:.3e}")
    assert got.shape == r64.shape and e_hip <= 4 * e_t32


def test_running_statistics_changed_in_place_are_folded_again(model, refs):
    """The stale-weight guard of the fold: a second call after an in-place change of a running mean gives the new result."""
    size = SIZES[0]
    img, _, _ = refs[size]
    bn = model.res2[0].conv1.norm
    before = model(img.cuda())["res2"].clone()
    saved = bn.running_mean.clone()
    try:
        bn.running_mean.add_(0.5)
        sd = {k: v.cpu() for k, v in model.state_dict().items()}
        with torch.no_grad():
            r64 = R.resnet50(img.double(), R.cast(sd, torch.float64))["res2"]
            r32 = R.resnet50(img, R.cast(sd, torch.float32))["res2"]
        after = model(img.cuda())["res2"]
        assert not torch.equal(after, before)
        assert R.rel_max_err(after, r64) <= 4 * R.rel_max_err(r32, r64)
        assert R.rel_max_err(before, r64) > 100 * R.rel_max_err(r32, r64)          # the old fold is far outside the bound
    finally:
        bn.running_mean.copy_(saved)
    assert torch.equal(model(img.cuda())["res2"], before)
