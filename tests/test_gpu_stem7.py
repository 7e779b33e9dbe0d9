"""GPU: the 7x7 / stride-2 / 3 -> 64 stem kernel (csrc/stem7.hip) behind mss_conv2d_forward_f32, alone.

  * exact: small-integer images and weights, scales in {0.5, 1, 2} and integer shifts -- every partial sum is an integer below
    2^24 (147 terms of at most 4 * 2 = 8), so the fp32 result must equal the float64 reference bit for bit;
  * poison: columns of y behind the 64 channels and one guard row before and after y keep their poison;
  * random data: |y - y64| <= 2 * 150 * 2^-24 * (sum |x||w|) * |scale| + 2^-23 * |y64| -- the forward bound of a 147-term fp32
    sum with one fused affine, doubled; derived, not measured;
  * the route label, and the neighbouring argument combinations that stay MSS_ERR_UNSUPPORTED."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import poison

pytestmark = pytest.mark.gpu

SHAPES = [(1, 7, 7), (2, 37, 51), (1, 64, 96), (3, 33, 130)]       # odd sizes and every border; > 1 tile each way, ragged last tile


def launch(img, weight, affine, relu, ldy, fill=float("nan")):
    """The stem through kernels._conv_launch into rows 1 .. rows of a [rows + 2, ldy] buffer filled with `fill`. Returns the buffer
    and (N, OH, OW)."""
    from multishiftseg_amd import kernels as K
    n, _, h, w = img.shape
    OH, OW = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    rows = n * OH * OW
    buf = torch.full((rows + 2, ldy), fill, device="cuda", dtype=torch.float32)
    y = K.Act(buf[1:rows + 1].view(n, OH, OW, ldy), 64)
    x = K.image_to_nhwc(img, Cp=4)
    K._conv_launch(x, K.packed_stem7(weight), y, OH, OW, 2, 1, 3, None, False, affine, relu, None)
    torch.cuda.synchronize()
    return buf, (n, OH, OW)


def reference(img, weight, affine, relu):
    y = F.conv2d(img.double().cpu(), weight.double().cpu(), stride=2, padding=3)
    if affine is not None:
        y = y * affine[0].double().cpu().view(1, -1, 1, 1) + affine[1].double().cpu().view(1, -1, 1, 1)
    return F.relu(y) if relu else y


def integer_case(shape, seed):
    g = torch.Generator().manual_seed(seed)
    n, h, w = shape
    img = torch.randint(-4, 5, (n, 3, h, w), generator=g).float().cuda()
    weight = torch.randint(-2, 3, (64, 3, 7, 7), generator=g).float().cuda()
    scale = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (64,), generator=g)].cuda()
    shift = torch.randint(-5, 6, (64,), generator=g).float().cuda()
    return img, weight, (scale, shift)


@pytest.mark.parametrize("ldy", [64, 80])
@pytest.mark.parametrize("shape", SHAPES)
def test_exact_on_integers(shape, ldy):
    img, weight, affine = integer_case(shape, 11 + shape[1])
    for aff in (None, affine):
        for relu in (False, True):
            buf, (n, OH, OW) = launch(img, weight, aff, relu, ldy)
            got = buf[1:-1].view(n, OH, OW, ldy)[..., :64].permute(0, 3, 1, 2).cpu()
            ref = reference(img, weight, aff, relu)
            assert ref.abs().max() < 2 ** 24 and ref.shape == got.shape
            assert torch.equal(got.double(), ref), (shape, ldy, aff is not None, relu, float((got.double() - ref).abs().max()))


@pytest.mark.parametrize("value", poison.POISONS)
@pytest.mark.parametrize("shape", SHAPES)
def test_padding_columns_and_guard_rows_keep_their_poison(shape, value):
    img, weight, affine = integer_case(shape, 5)
    buf, _ = launch(img, weight, affine, True, 80, fill=value)
    host = buf.cpu()

    def untouched(t):
        return bool(torch.isnan(t).all()) if value != value else bool((t == value).all())
    assert untouched(host[0]) and untouched(host[-1])
    assert untouched(host[1:-1, 64:])
    assert bool(torch.isfinite(host[1:-1, :64]).all()) and float(host[1:-1, :64].abs().max()) < 1e20


def test_wrapper_under_poisoned_allocations():
    """kernels.stem7_conv end to end with every scratch buffer poisoned: the image's pad channel is written, not assumed."""
    from multishiftseg_amd import kernels as K
    img, weight, affine = integer_case((2, 37, 51), 9)
    poison.poison_runs(lambda: K.stem7_conv(img, weight, affine, relu=True).buf, bitwise=True)


@pytest.mark.parametrize("shape", SHAPES)
def test_random_data_within_the_forward_bound(shape):
    g = torch.Generator().manual_seed(100 + shape[2])
    n, h, w = shape
    img = torch.randn((n, 3, h, w), generator=g).cuda()
    weight = (torch.randn((64, 3, 7, 7), generator=g) / 12).cuda()
    scale = (torch.rand(64, generator=g) + 0.5).cuda() * torch.where(torch.rand(64, generator=g) < 0.25, -1.0, 1.0).cuda()
    shift = (torch.rand(64, generator=g) - 0.5).cuda()
    for aff in (None, (scale, shift)):
        buf, (n_, OH, OW) = launch(img, weight, aff, False, 64)
        got = buf[1:-1].view(n_, OH, OW, 64).permute(0, 3, 1, 2).cpu().double()
        ref = reference(img, weight, aff, False)
        mag = F.conv2d(img.double().cpu().abs(), weight.double().cpu().abs(), stride=2, padding=3)
        sc = torch.ones(64, dtype=torch.float64) if aff is None else scale.double().cpu().abs()
        bound = 2 * 150 * 2.0 ** -24 * mag * sc.view(1, -1, 1, 1) + 2.0 ** -23 * ref.abs()
        worst = float(((got - ref).abs() / bound).max())
        print(f"stem7 random {shape} affine={aff is not None}: max err / bound = {worst:.3f}")
        assert worst <= 1.0


def _args(img, weight, ldy=64, Cp=4):
    from multishiftseg_amd import kernels as K
    n, _, h, w = img.shape
    OH, OW = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    x = K.image_to_nhwc(img, Cp=Cp)
    y = K.Act.empty(n, h, w, 64, img.device, ld=ldy)                 # room for a stride-1 output too: nothing below may overrun it
    if Cp == 4:
        pw = K.packed_stem7(weight)
    else:
        t = torch.zeros((49, 64, Cp), device="cuda")
        pw = K.PackedWeight(t, 64, 3, 7, 7, 64, Cp)
    a = K._conv_args(x, pw, y, 2, 1, 3, None, False, None, False, None)
    a.OH, a.OW, a.ldy = OH, OW, ldy
    return a, (x, y, pw)


def test_route_label_and_unsupported_neighbours():
    from multishiftseg_amd import _lib
    img, weight, _ = integer_case((1, 64, 96), 3)
    a, keep = _args(img, weight)
    assert _lib.value("mss_conv2d_forward_route", ctypes.byref(a)) == 5
    assert _lib.status("mss_conv2d_forward_f32", ctypes.byref(a)) == 0

    a, keep = _args(img, weight)
    a.stride, a.OH, a.OW = 1, 64, 96
    assert _lib.value("mss_conv2d_forward_route", ctypes.byref(a)) != 5
    assert _lib.status("mss_conv2d_forward_f32", ctypes.byref(a)) == _lib.MSS_ERR_UNSUPPORTED

    a, keep = _args(img, weight, Cp=16)
    assert _lib.value("mss_conv2d_forward_route", ctypes.byref(a)) != 5
    assert _lib.status("mss_conv2d_forward_f32", ctypes.byref(a)) == _lib.MSS_ERR_UNSUPPORTED

    a, keep = _args(img, weight)
    ones, zeros = torch.ones(16, device="cuda"), torch.zeros(16, device="cuda")
    a.in_scale, a.in_shift = _lib.ptr(ones), _lib.ptr(zeros)
    assert _lib.value("mss_conv2d_forward_route", ctypes.byref(a)) != 5
    assert _lib.status("mss_conv2d_forward_f32", ctypes.byref(a)) == _lib.MSS_ERR_UNSUPPORTED
    torch.cuda.synchronize()
