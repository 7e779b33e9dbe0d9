"""GPU: the stem's weight-gradient kernel alone (csrc/stem7_wgrad.hip through kernels.stem7_wgrad), plain and with the max-pool +
ReLU backward fused, against stock torch in float64 on the CPU.

Exact cases: small integers, so every partial sum is an integer far below 2^24 and the result is the same in any summation order --
torch.equal with the float64 gradient. The pool form's a0 takes values in {0, 1, 2, 3}, a third of them zero, so most windows hold a
positive TIE (also across window rows and at the border): the arg-max rule (first maximum in row-major order, F.max_pool2d's) decides
the result there. Random cases: e = max|G - G64| / max|G64| against the same figure of stock torch float32 on the CPU, under the
project's one-kernel factor 4 (FACTOR of tests/test_gpu_resnet_backward.py)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import poison
import ref_resnet as R
from test_stem7_wgrad_cpu import LONG, MULTI, STEM_SIZES, ask, stem_args

pytestmark = pytest.mark.gpu

FACTOR = 4
RANDOM_SIZES = ((1, 70, 100), (2, 64, 96), MULTI)


def _grid(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def wgrad_ref(img, dz, dtype):
    """The weight gradient of F.conv2d(img, w, stride 2, padding 3) at dz, stock torch on the CPU."""
    w = torch.zeros((64, 3, 7, 7), dtype=dtype, requires_grad=True)
    (F.conv2d(img.to(dtype), w, None, 2, 3) * dz.to(dtype)).sum().backward()
    return w.grad


def pool_dz_ref(a0, dy, dtype):
    """Autograd of F.max_pool2d(F.relu(z), 3, 2, 1) at z = a0: the gradient at the stem convolution's normed output."""
    z = a0.to(dtype).clone().requires_grad_(True)
    (F.max_pool2d(F.relu(z), 3, 2, 1) * dy.to(dtype)).sum().backward()
    return z.grad


def windows(a0):
    """a0 [N, C, OH, OW] -> ([N*C, 9, L] window values with -inf outside the map, [N*C, 1, L] maxima)."""
    n, c, oh, ow = a0.shape
    u = F.unfold(F.pad(a0.reshape(n * c, 1, oh, ow), (1, 1, 1, 1), value=float("-inf")), 3, stride=2)
    return u, u.max(1, keepdim=True).values


def positive_ties(a0):
    u, mx = windows(a0)
    return ((u == mx) & (mx > 0)).sum(1) > 1                # [N*C, L]


def exact_case(size, pool):
    n, h, w = size
    oh, ow = _grid(h, w)
    g = torch.Generator().manual_seed(1000 * h + w + (7 if pool else 0))
    img = torch.randint(-4, 5, (n, 3, h, w), generator=g).float()
    if not pool:
        return img, torch.randint(-3, 4, (n, 64, oh, ow), generator=g).float(), None
    a0 = torch.randint(0, 9, (n, 64, oh, ow), generator=g)
    a0 = torch.where(a0 < 3, torch.zeros_like(a0), (a0 - 3) // 2 + 1).float()          # 0 with 1/3, 1 / 2 / 3 with 2/9 each
    dy = torch.randint(-3, 4, (n, 64) + _grid(oh, ow), generator=g).float()
    return img, dy, a0


def run(img, dy, a0=None, ld=None):
    from multishiftseg_amd import kernels as K

    def act(t):
        a = K.Act.from_nchw(t.cuda(), ld=ld)
        if ld:
            a.buf[..., t.shape[1]:] = float("nan")
        return a
    return K.stem7_wgrad(img.cuda(), act(dy), None if a0 is None else act(a0))


def test_unpack_takes_the_49_tap_pack():
    """mss_conv2d_unpack_wgrad_f32(K = 64, C = 3, R = S = 7, Kpad = 64, Cp = 4) inverts the forward's pack."""
    from multishiftseg_amd import kernels as K
    from multishiftseg_amd._lib import call, ptr
    w = torch.randn((64, 3, 7, 7), generator=torch.Generator().manual_seed(3)).cuda()
    packed = torch.full((49, 64, 4), float("nan"), device="cuda")
    call("mss_conv2d_pack_weights_f32", ptr(w), ptr(packed), 64, 3, 7, 7, 64, 4, 0, None, 0, 0)
    assert torch.equal(packed[:, :, :3], w.permute(2, 3, 0, 1).reshape(49, 64, 3)) and bool((packed[:, :, 3] == 0).all())
    back = torch.full((64, 3, 7, 7), float("nan"), device="cuda")
    call("mss_conv2d_unpack_wgrad_f32", ptr(packed), ptr(back), 64, 3, 7, 7, 64, 4, 0, None, None, 0, 0)
    assert torch.equal(back, w)


@pytest.mark.parametrize("size", STEM_SIZES + (LONG,), ids=str)
def test_plain_form_exact(size):
    if size in (MULTI, LONG):
        rc, plan = ask(stem_args(*size))
        assert rc == 0 and plan.splits > 1
    img, dz, _ = exact_case(size, False)
    bound = 4 * 3 * dz[0, 0].numel() * size[0]
    assert bound < 2 ** 24
    got = run(img, dz)
    assert torch.equal(got.cpu().double(), wgrad_ref(img, dz, torch.float64))


@pytest.mark.parametrize("size", STEM_SIZES + (LONG,), ids=str)
def test_pool_form_exact_with_ties(size):
    if size in (MULTI, LONG):
        rc, plan = ask(stem_args(*size, pool=True))
        assert rc == 0 and plan.splits > 1
    img, dy, a0 = exact_case(size, True)
    n, _, oh, ow = a0.shape
    ph, pw = _grid(oh, ow)
    # what the data is for: positive ties in most windows, across window rows, and in the border windows
    ties = positive_ties(a0)
    u, mx = windows(a0)
    hit = (u == mx) & (mx > 0)
    rows = (hit[:, 0:3].any(1).int() + hit[:, 3:6].any(1).int() + hit[:, 6:9].any(1).int()) > 1
    border = torch.zeros(ph, pw, dtype=torch.bool)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    zeros = float((a0 == 0).float().mean())
    print(f"{size}: {float(ties.float().mean()):.2f} of the windows hold a positive tie, {float(rows.float().mean()):.2f} one across rows, "
          f"{float(ties[:, border.flatten()].float().mean()):.2f} of the border windows; {zeros:.2f} zeros")
    assert ties.float().mean() > 0.5 and rows.any() and ties[:, border.flatten()].any() and 0.25 < zeros < 0.42
    dz = pool_dz_ref(a0, dy, torch.float64)
    assert dz.abs().max() <= 12 and 4 * 12 * dz[0, 0].numel() * n < 2 ** 24
    got = run(img, dy, a0)
    assert torch.equal(got.cpu().double(), wgrad_ref(img, dz, torch.float64))


@pytest.mark.parametrize("size", RANDOM_SIZES, ids=str)
@pytest.mark.parametrize("pool", [False, True], ids=["plain", "pool"])
def test_random_data_within_the_one_kernel_factor(size, pool):
    n, h, w = size
    oh, ow = _grid(h, w)
    g = torch.Generator().manual_seed(31 * h + w + int(pool))
    img = torch.randn((n, 3, h, w), generator=g)
    if pool:
        a0 = F.relu(torch.randn((n, 64, oh, ow), generator=g))
        dy = torch.randn((n, 64) + _grid(oh, ow), generator=g)
        # conditions, not tolerances: no positive tie, and the same arg-max in float32 and float64 wherever the maximum is positive
        assert not positive_ties(a0).any()
        m32, i32 = F.max_pool2d(a0, 3, 2, 1, return_indices=True)
        m64, i64 = F.max_pool2d(a0.double(), 3, 2, 1, return_indices=True)
        assert torch.equal(i32[m64 > 0], i64[m64 > 0]) and torch.equal(m32 > 0, m64 > 0)
        dz64, dz32 = pool_dz_ref(a0, dy, torch.float64), pool_dz_ref(a0, dy, torch.float32)
        got = run(img, dy, a0)
    else:
        dz64 = torch.randn((n, 64, oh, ow), generator=g)
        dz32 = dz64
        got = run(img, dz64)
    g64, g32 = wgrad_ref(img, dz64, torch.float64), wgrad_ref(img, dz32, torch.float32)
    e_hip, e_t32 = R.rel_max_err(got, g64), R.rel_max_err(g32, g64)
    print(f"{size} {'pool' if pool else 'plain'}: e_hip {e_hip:.3e}  e_t32 {e_t32:.3e}  ratio {e_hip / e_t32:.2f}")
    assert e_hip <= FACTOR * e_t32


@pytest.mark.parametrize("pool", [False, True], ids=["plain", "pool"])
def test_pitches_poison_and_reproducibility(pool):
    """lddy and ldres above 64 with NaN in the pad columns; dwp, the scratch slabs and every other buffer the wrapper allocates
    pre-filled with NaN, then with 1e30: bitwise the dense clean result, finite, and the same bits run to run."""
    img, dy, a0 = exact_case(MULTI, pool)
    rc, plan = ask(stem_args(*MULTI, pool=pool), lddy=72)
    assert rc == 0 and plan.splits > 1 and plan.ws_bytes > 0
    dense = run(img, dy, a0).cpu()
    runs = poison.poison_runs(lambda: run(img, dy, a0, ld=72), bitwise=True)
    for tag in ("clean", "clean2") + poison.POISONS:
        assert torch.equal(runs[tag][0], dense) and bool(torch.isfinite(runs[tag][0]).all()), tag


def test_the_launch_refuses_a_short_scratch():
    from multishiftseg_amd import _lib, kernels as K
    img, dz, _ = exact_case(MULTI, False)
    x = K.image_to_nhwc(img.cuda(), Cp=4)
    dy = K.Act.from_nchw(dz.cuda())
    a = stem_args(*MULTI, x=x.ptr)
    need = _lib.value("mss_conv2d_wgrad_workspace_bytes", ctypes.byref(a), 4)
    assert need > 0
    dwp = torch.zeros((49, 64, 4), device="cuda")
    ws = torch.zeros(need // 4, device="cuda")
    short = _lib.status("mss_conv2d_wgrad_f32", ctypes.byref(a), dy.ptr, dy.ld, _lib.ptr(dwp), 4, _lib.ptr(ws), need - 4)
    assert short == _lib.MSS_ERR_BAD_ARG and not dwp.any()
    assert _lib.status("mss_conv2d_wgrad_f32", ctypes.byref(a), dy.ptr, dy.ld, _lib.ptr(dwp), 4, None, 0) == _lib.MSS_ERR_BAD_ARG
