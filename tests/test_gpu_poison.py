"""Every kernel wrapper on dirty memory (tests/poison.py): each case runs the call under test twice clean and once with every
torch.empty / empty_like / new_empty buffer filled with NaN and once with +1e30 (split-bf16 weight planes with 0xFF). The
poisoned outputs must be finite, equal the clean run bit for bit wherever two clean runs agree bit for bit, and meet the
float64 / reference-fixture bound of the family's own test (tests/test_gpu_ops.py and friends). Models, parameters and
inputs are built outside the poison; packed weights are dropped before every run, so the packs are made inside it.

Act inputs live in wider buffers whose columns outside the window the wrapper reads are NaN; Act outputs are written into
windows of NaN buffers whose outside must come back untouched."""
import ast

import numpy as np
import pytest
import torch

from conftest import golden
from oracle import msda as omsda
from poison import poison_runs

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def K():
    from multishiftseg_amd import kernels
    return kernels


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def each_run(r):
    return [v for k, v in r.items() if k != "reproducible"]


def window_act(K, x_nchw, c0=4, read=None, extra=8):
    """Act of x (NCHW numpy) at channel offset c0 of a NaN buffer; columns [c0 + C, c0 + read) zero (the pad the wrapper may read)."""
    n, c, h, w = x_nchw.shape
    read = read or c
    ld = -(-(c0 + read + extra) // 4) * 4
    buf = torch.full((n, h, w, ld), NAN, device="cuda")
    buf[..., c0:c0 + c] = dev(x_nchw).permute(0, 2, 3, 1)
    buf[..., c0 + c:c0 + read] = 0
    return K.Act(buf, c, c0)


def out_window(K, n, h, w, c, c0=8, extra=12):
    ld = -(-(c0 + c + extra) // 4) * 4
    return K.Act(torch.full((n, h, w, ld), NAN, device="cuda"), c, c0)


def outside_untouched(a):
    """The columns of a's buffer outside its window are still NaN."""
    b = a.buf
    return bool(torch.isnan(b[..., :a.c0]).all()) and bool(torch.isnan(b[..., a.c0 + a.C:]).all())


def drop_packs(*params):
    for p in params:
        p.__dict__.pop("_mss_packed", None)


def f64_conv(x, w, stride=1, dil=1, pad=0):
    return torch.nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(w).double(), stride=stride, dilation=dil,
                                      padding=pad).numpy()


def close(got, ref, rtol, atol, msg=""):
    np.testing.assert_allclose(got.numpy() if isinstance(got, torch.Tensor) else got, ref, rtol=rtol, atol=atol, err_msg=msg)


def new_bn(c, seed):
    g = torch.Generator().manual_seed(seed)
    bn = torch.nn.BatchNorm2d(c)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(c, generator=g))
        bn.running_mean.copy_(torch.randn(c, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(c, generator=g) + 0.5)
    return bn.cuda()


def bn_reset(bn, saved):
    def setup():
        bn.load_state_dict(saved)
    return setup


def check_bn(st, y_ref, bn_ref, rtol=1e-4):
    """save_mean / save_invstd / running statistics of a train-mode fold against float64 statistics of y_ref (NCHW)."""
    m = y_ref.mean((0, 2, 3))
    v = y_ref.var((0, 2, 3))
    n = y_ref.size // y_ref.shape[1]
    eps = 1e-5
    mean, invstd, rm, rv = st
    close(mean, m, rtol, 1e-4)
    close(invstd, 1 / np.sqrt(v + eps), 1e-3, 1e-4)
    close(rm, 0.9 * bn_ref[0] + 0.1 * m, rtol, 1e-4)
    close(rv, 0.9 * bn_ref[1] + 0.1 * v * n / (n - 1), 1e-3, 1e-4)


# ---- convolutions ------------------------------------------------------------------------------------------------------------
CONV_CASES = [
    # cin, cout, r, stride, dil, n, h, w
    (40, 136, 1, 1, 1, 2, 17, 19),      # 1x1 persistent GEMM; Cp 48 (pad 8), K 136 (not a multiple of 128)
    (36, 100, 3, 1, 2, 2, 11, 13),      # implicit GEMM, dilation 2, Cp 48, ragged rows
    (20, 68, 3, 2, 1, 2, 17, 19),       # stride 2, Cp 32
    (52, 304, 3, 1, 1, 1, 12, 10),      # tail pack 304 = 2 x 128 + 48
    (24, 48, 1, 1, 1, 1, 9, 7),         # narrow 64-wide tile, 63 rows
    (520, 100, 1, 1, 1, 1, 1, 3),       # few-rows route (3 rows)
    (300, 19, 1, 1, 1, 2, 5, 6),        # 19 output channels (the heads), Cp 304
]


@pytest.mark.parametrize("cin,cout,r,stride,dil,n,h,w", CONV_CASES)
def test_conv_forward_with_stats(K, cin, cout, r, stride, dil, n, h, w, gemm_route):
    """conv2d (pack made inside the poison) from a channel window into an output window, with the epilogue's BatchNorm partial
    sums folded by bn_fold(train=True): output vs float64 (rtol / atol 1e-4, test_conv_vs_oracle), statistics vs float64."""
    rng = np.random.default_rng(cin * 7 + cout + r)
    x = rng.standard_normal((n, cin, h, w), dtype=np.float32)
    wt = (rng.standard_normal((cout, cin, r, r), dtype=np.float32) / np.sqrt(cin * r * r)).astype(np.float32)
    pad = dil if r == 3 else 0
    ref = f64_conv(x, wt, stride, dil, pad)
    cp = -(-cin // 16) * 16
    xa = window_act(K, x, read=cp)
    wd = dev(wt)
    bn = new_bn(cout, 1)
    saved = {k: v.clone() for k, v in bn.state_dict().items()}
    tail = cout % 128 and cout > 128 and cout % 128 <= 64
    fold = not tail and cout % 4 == 0           # the BatchNorm statistics kernels take channel quads

    def run():
        y = K.conv2d(xa, K.pack_weight(wd), stride=stride, dil=dil, pad=pad, out=out_window(K, n, ref.shape[2], ref.shape[3], cout),
                     want_stats=True)
        assert outside_untouched(y)
        outs = [y.nchw()]
        if not tail:
            assert y.stats is not None
            outs.append(y.stats[:, 0].double().sum(0))
        if fold:
            st = K.bn_fold(bn, y, train=True)
            outs += [st.save_mean, st.save_invstd, bn.running_mean, bn.running_var, st.scale, st.shift]
        return outs

    r_ = poison_runs(run, setup=bn_reset(bn, saved))
    for o in each_run(r_):
        close(o[0], ref, 1e-4, 1e-4)
        if not tail:
            close(o[1], ref.sum((0, 2, 3)), 1e-4, 1e-2)
        if fold:
            check_bn(o[2:6], ref, (saved["running_mean"].cpu().numpy(), saved["running_var"].cpu().numpy()))


@pytest.mark.parametrize("tile", [2, 4, 6])
@pytest.mark.parametrize("cin,cout,dil,n,h,w", [(32, 36, 1, 2, 13, 11), (48, 100, 2, 1, 14, 19), (64, 304, 1, 1, 9, 10),
                                                (16, 132, 3, 1, 7, 23)])
def test_winograd_forward_with_stats(K, cin, cout, dil, n, h, w, tile, gemm_route):
    """conv2d_winograd with the BatchNorm+ReLU prologue, a residual and the output transform's partial sums, ragged H / W for the
    tile, output channels that leave padded Winograd-domain rows (36, 100, 132) and the 304 tail; output vs float64 (1e-4)."""
    rng = np.random.default_rng(cin + cout + dil + tile)
    x = rng.standard_normal((n, cin, h, w), dtype=np.float32)
    wt = (rng.standard_normal((cout, cin, 3, 3), dtype=np.float32) / np.sqrt(cin * 9)).astype(np.float32)
    sc = rng.uniform(0.5, 1.5, cin).astype(np.float32)
    sh = rng.standard_normal(cin).astype(np.float32)
    res = rng.standard_normal((n, cout, h, w), dtype=np.float32)
    act = np.maximum(x * sc[None, :, None, None] + sh[None, :, None, None], 0)
    ref = f64_conv(act, wt, 1, dil, dil) + res
    xa, ra = window_act(K, x), window_act(K, res, c0=0)
    wd, scd, shd = dev(wt), dev(sc), dev(sh)
    bn = new_bn(cout, 2)
    saved = {k: v.clone() for k, v in bn.state_dict().items()}

    def run():
        y = K.conv2d_winograd(xa, K.pack_weight_wino(wd, tile=tile), dil=dil, in_affine=(scd, shd), in_relu=True, res=ra,
                              want_stats=True)
        assert y.stats is not None
        st = K.bn_fold(bn, y, train=True)
        return [y.nchw(), st.save_mean, st.save_invstd, bn.running_mean, bn.running_var]

    r_ = poison_runs(run, setup=bn_reset(bn, saved))
    for o in each_run(r_):
        close(o[0], ref, 1e-4, 1e-4)
        check_bn(o[1:5], ref, (saved["running_mean"].cpu().numpy(), saved["running_var"].cpu().numpy()))


@pytest.mark.parametrize("tile", [4, 6])
def test_winograd_pair_and_aspp_transform(K, tile, gemm_route):
    """conv3x3_pair (two dilated layers, one batched launch, packed pair made inside the poison) and the fused ASPP input
    transform feeding conv3x3(xt=...): vs float64 (1e-4), statistics folded."""
    torch.manual_seed(tile)
    n, h, w, c, k = 1, 24, 24, 64, 128
    from multishiftseg_amd import _lib
    assert _lib.value("mss_wino_num_tiles", n, h, w, 1, tile) == _lib.value("mss_wino_num_tiles", n, h, w, 2, tile)
    x = torch.randn(n, c, h, w)
    w1, w2, w3 = (torch.nn.Parameter(torch.randn(k, c, 3, 3, device="cuda") * 0.05) for _ in range(3))
    xa = window_act(K, x.numpy(), c0=0, extra=0)
    refs = [f64_conv(x.numpy(), p.detach().cpu().numpy(), 1, d, d) for p, d in ((w1, 1), (w2, 2), (w3, 3))]

    def run():
        drop_packs(w1, w2, w3)
        o1, o2 = out_window(K, n, h, w, k, c0=0), out_window(K, n, h, w, k, c0=0)
        K.conv3x3_pair(xa, w1, w2, 1, 2, o1, o2, tile, want_stats=True)
        outs = [o1.nchw(), o2.nchw(), o1.stats, o2.stats]
        plan = K.aspp_plan_for(xa, (1, 2, 3), (w1, w2, w3))
        if plan.single_read:
            for p, d, xt in zip((w1, w2, w3), (1, 2, 3), K.aspp_transforms(xa, (1, 2, 3), plan)[0].xts):
                outs.append(K.conv3x3(xa, p, dil=d, xt=xt).nchw())
        return outs

    r_ = poison_runs(run)
    for o in each_run(r_):
        close(o[0], refs[0], 1e-4, 1e-4)
        close(o[1], refs[1], 1e-4, 1e-4)
        close(o[2][:, 0].double().sum(0), refs[0].sum((0, 2, 3)), 1e-4, 1e-2)
        for got, ref in zip(o[4:], refs):
            close(got, ref, 1e-4, 1e-4)


@pytest.mark.parametrize("cin,cout,r,dil,n,h,w", [(64, 128, 3, 1, 2, 14, 13), (256, 48, 1, 1, 1, 9, 8), (128, 64, 3, 12, 1, 20, 18),
                                                  (304, 100, 3, 1, 1, 11, 9), (48, 36, 3, 2, 2, 10, 7)])
def test_dgrad_and_wgrad(K, cin, cout, r, dil, n, h, w, gemm_route):
    """Data gradient (flipped pack, also through conv3x3's Winograd / direct choice) and the direct weight gradient (dwp
    fully overwritten by the kernel) from a gradient that is a channel window of a wider buffer; vs float64 autograd
    (1e-4 / 1e-3, test_dgrad_and_wgrad)."""
    rng = np.random.default_rng(cin + cout + dil)
    pad = dil if r == 3 else 0
    x = torch.from_numpy(rng.standard_normal((n, cin, h, w), dtype=np.float32)).double().requires_grad_(True)
    wt = torch.from_numpy((rng.standard_normal((cout, cin, r, r)) / np.sqrt(cin * r * r)).astype(np.float32)).double().requires_grad_(True)
    y = torch.nn.functional.conv2d(x, wt, dilation=dil, padding=pad)
    gy = rng.standard_normal(tuple(y.shape), dtype=np.float32)
    y.backward(torch.from_numpy(gy).double())
    kp = -(-cout // 16) * 16
    ga = window_act(K, gy, read=kp)
    xa = window_act(K, x.detach().float().numpy())
    wp = torch.nn.Parameter(wt.detach().float().cuda())

    def run():
        drop_packs(wp)
        dx = K.conv2d(ga, K.pack_weight(wp.detach(), flip=True), dil=dil, pad=pad)
        dw = K.conv2d_wgrad(xa, ga, cout, cin, r, r, dil=dil, pad=pad)
        outs = [dx.nchw(), dw]
        if r == 3 and cout % 16 == 0:
            outs.append(K.conv3x3(ga, wp, dil=dil, flip=True).nchw())
        if r == 3:
            outs.append(K.conv3x3_wgrad(xa, ga, cout, cin, dil=dil))
        return outs

    r_ = poison_runs(run)
    for o in each_run(r_):
        close(o[0], x.grad.numpy(), 1e-4, 1e-4)
        close(o[1], wt.grad.numpy(), 1e-3, 1e-3)
        if r == 3:
            close(o[-1], wt.grad.numpy(), 1e-3, 1e-3)
            if cout % 16 == 0:
                close(o[2], x.grad.numpy(), 1e-4, 1e-4)


WGRAD_ROUTES = [
    # mode (MSS_WGRAD_TN), P, T, C, Ko: the batched Winograd-domain weight-gradient kernels (test_batched_wgrad_routes_vs_float64)
    ("0", 3, 700, 512, 128), ("1", 2, 1000, 256, 72), ("1", 4, 37, 768, 256), ("4", 3, 700, 512, 128), ("4", 2, 1000, 256, 72),
    ("7", 4, 37, 768, 256), ("5", 36, 1100, 1024, 256),
]


@pytest.mark.parametrize("mode,P,T,C,Ko", WGRAD_ROUTES)
def test_batched_wgrad_routes(K, monkeypatch, mode, P, T, C, Ko):
    """dU = dY'^T X' on every batched TN kernel (the split TN kernel runs in test_dgrad_and_wgrad), its pixel-split workspace and
    `du` made inside the poison: every element of du written, vs float64 (test_batched_wgrad_routes_vs_float64)."""
    import ctypes
    from multishiftseg_amd._lib import MssConvArgs, call, ptr
    monkeypatch.setenv("MSS_WGRAD_TN", mode)
    torch.manual_seed(P * T + C)
    xt = torch.randn(P, T, C, device="cuda")
    dyt = torch.randn(P, T, Ko, device="cuda")
    kpad = (Ko + 3) // 4 * 4

    def run():
        a = MssConvArgs()
        a.x = ptr(xt)
        a.N, a.H, a.W, a.C, a.ldx = 1, 1, T, C, C
        a.OH, a.OW, a.K, a.Kpad = 1, T, Ko, kpad
        a.R, a.S, a.stride, a.dil, a.pad = 1, 1, 1, 1, 0
        a.batch, a.x_bs, a.y_bs = P, T * C, T * Ko
        du = torch.empty((P, kpad, C), device="cuda")
        ws, wsb = K._wgrad_workspace(a, C, "cuda")
        call("mss_conv2d_wgrad_f32", ctypes.byref(a), ptr(dyt), Ko, ptr(du), C, ptr(ws), wsb)
        return du[:, :Ko]

    r_ = poison_runs(run)
    want = torch.einsum("ptk,ptc->pkc", dyt.double(), xt.double()).cpu()
    for o in each_run(r_):
        assert (o[0].double() - want).abs().max().item() <= 2e-6 * T ** 0.5 * 16


@pytest.mark.parametrize("n,h,w,cin,k,ld,c0,affine", [(1, 128, 160, 256, 19, 48, 20, True), (2, 96, 100, 128, 48, 48, 0, False),
                                                     (1, 130, 131, 256, 20, 20, 0, True), (1, 128, 129, 384, 34, 36, 0, True)])
def test_narrow_and_direct_wgrad(K, n, h, w, cin, k, ld, c0, affine, gemm_route):
    """1x1 weight gradients with <= 64 output channels (narrow kernel, a slice of the 48-wide head gradient) and the direct
    kernel with the BatchNorm+ReLU prologue, dwp and the pixel-split workspace made inside the poison; vs float64."""
    torch.manual_seed(n * h + k)
    x = torch.randn(n, h, w, cin, device="cuda")
    gbuf = torch.randn(n, h, w, ld, device="cuda")
    sc, sh = torch.rand(cin, device="cuda") + 0.5, torch.randn(cin, device="cuda")
    xa, ga = K.Act(x), K.Act(gbuf, k, c0)
    aff = (sc, sh) if affine else None

    def run():
        return K.conv2d_wgrad(xa, ga, k, cin, 1, 1, in_affine=aff, in_relu=affine)

    r_ = poison_runs(run)
    xv = torch.relu(x.double() * sc.double() + sh.double()) if affine else x.double()
    want = torch.einsum("nhwk,nhwc->kc", gbuf[..., c0:c0 + k].double(), xv).cpu()[:, :, None, None]
    for o in each_run(r_):
        assert (o[0].double() - want).abs().max().item() <= 1e-5 * (n * h * w) ** 0.5 * 4


@pytest.mark.parametrize("P,T,C,Ko,tail", [(36, 1100, 4096, 256, "1"), (9, 777, 2048, 1024, "0")])
def test_direct_wgrad_tail_plan(K, monkeypatch, P, T, C, Ko, tail):
    """The direct TN kernel's tail plan (whole rounds unsplit, the rest cut into row ranges) and its all-split form."""
    import ctypes
    from multishiftseg_amd._lib import MssConvArgs, call, ptr
    monkeypatch.setenv("MSS_WGRAD_TN", "7")
    monkeypatch.setenv("MSS_WGRAD_TN_TAIL", tail)
    torch.manual_seed(P + T)
    xt = torch.randn(P, T, C, device="cuda")
    dyt = torch.randn(P, T, Ko, device="cuda")

    def run():
        a = MssConvArgs()
        a.x = ptr(xt)
        a.N, a.H, a.W, a.C, a.ldx = 1, 1, T, C, C
        a.OH, a.OW, a.K, a.Kpad = 1, T, Ko, Ko
        a.R, a.S, a.stride, a.dil, a.pad = 1, 1, 1, 1, 0
        a.batch, a.x_bs, a.y_bs = P, T * C, T * Ko
        du = torch.empty((P, Ko, C), device="cuda")
        ws, wsb = K._wgrad_workspace(a, C, "cuda")
        call("mss_conv2d_wgrad_f32", ctypes.byref(a), ptr(dyt), Ko, ptr(du), C, ptr(ws), wsb)
        return du

    r_ = poison_runs(run)
    want = torch.einsum("ptk,ptc->pkc", dyt.double(), xt.double()).cpu()
    for o in each_run(r_):
        assert (o[0].double() - want).abs().max().item() <= 2e-6 * T ** 0.5 * 16


@pytest.mark.parametrize("n,h,w,cin,cout", [(2, 40, 56, 128, 128), (1, 24, 26, 256, 304)])
def test_dgrad_after_bn_fused(K, n, h, w, cin, cout, gemm_route):
    """conv3x3_dgrad_after_bn (the BatchNorm+ReLU backward folded into the Winograd input transform of the data gradient of the
    cout -> cin layer in front of it): vs float64 autograd on the same BatchNorm input (relative L2 2e-4, as
    test_dgrad_after_bn_fused_equals_separate_steps)."""
    torch.manual_seed(n * h + cin)
    wt = torch.nn.Parameter(torch.randn(cin, cout, 3, 3, device="cuda") * 0.05)
    bn = new_bn(cin, 3)
    x = torch.randn(n, cin, h, w, device="cuda") * 2 + 0.3
    gy = torch.randn(n, cin, h, w, device="cuda")
    xa, ga = window_act(K, x.cpu().numpy(), c0=0, extra=0), window_act(K, gy.cpu().numpy(), c0=0, extra=0)
    st = K.bn_fold(bn, xa, train=True)
    xq = x.double().requires_grad_(True)
    torch.relu(torch.nn.functional.batch_norm(xq, None, None, bn.weight.detach().double(), bn.bias.detach().double(),
                                              training=True)).backward(gy.double())
    want = torch.nn.functional.conv_transpose2d(xq.grad, wt.detach().double(), padding=1).cpu()

    def run():
        drop_packs(wt)
        return K.conv3x3_dgrad_after_bn(ga, xa, st, wt).nchw()

    r_ = poison_runs(run)
    for o in each_run(r_):
        assert (o[0].double() - want).norm().item() <= 2e-4 * want.norm().item()


# ---- BatchNorm ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,n,h,w", [(16, 3, 9, 7), (36, 2, 13, 11), (100, 1, 1, 65)])
def test_bn_fold_reread_and_relu_backward(K, c, n, h, w):
    """bn_fold(train=True) from a statistics pass over a channel window, the [M, C] row form, and the BN+ReLU backward with
    parameter gradients (its _col_accum workspace and dx made inside the poison); vs float64 autograd (test_bn_relu_backward)."""
    rng = np.random.default_rng(c)
    x = rng.standard_normal((n, c, h, w), dtype=np.float32) * 2 + 0.3
    gy = rng.standard_normal((n, c, h, w), dtype=np.float32)
    bn = new_bn(c, 4)
    saved = {k: v.clone() for k, v in bn.state_dict().items()}
    xd = torch.from_numpy(x).double().requires_grad_(True)
    gam = bn.weight.detach().cpu().double().requires_grad_(True)
    bet = bn.bias.detach().cpu().double().requires_grad_(True)
    torch.relu(torch.nn.functional.batch_norm(xd, None, None, gam, bet, training=True)).backward(torch.from_numpy(gy).double())
    xa, ga = window_act(K, x), window_act(K, gy)
    rows = dev(x.transpose(0, 2, 3, 1).reshape(-1, c))

    def run():
        st = K.bn_fold(bn, xa, train=True)
        dx, dg, db = K.bn_relu_backward(ga, xa, st, want_param_grads=True)
        st2 = K.bn_fold(bn, x_rows=rows, train=True)
        return [dx.nchw(), dg, db, st.save_mean, st.save_invstd, st2.scale, st2.shift, st.scale, st.shift]

    r_ = poison_runs(run, setup=bn_reset(bn, saved))
    for o in each_run(r_):
        close(o[0], xd.grad.numpy(), 1e-4, 1e-5)
        close(o[1], gam.grad.numpy(), 1e-4, 1e-4)
        close(o[2], bet.grad.numpy(), 1e-4, 1e-4)
        close(o[3], x.astype(np.float64).mean((0, 2, 3)), 1e-5, 1e-5)
        close(o[5], o[7].numpy(), 1e-5, 1e-6)
        close(o[6], o[8].numpy(), 1e-5, 1e-5)


# ---- glue and norms ----------------------------------------------------------------------------------------------------------
def test_pool_gap_upsample_stem_layout(K):
    """maxpool3s2 (NaN-free under +1e30: a read of unwritten memory would win the max), GAP by a pass and from the producer's
    partial sums, colsum, align-corners upsample forward / backward, the fused stem, the im2col stem, NCHW -> NHWC with
    channel padding; vs float64 / the reference's vectors."""
    g = golden("ops")
    rng = np.random.default_rng(2)
    px = g["pool_x"]
    ux = g["up_x"]
    x = rng.standard_normal((3, 64, 5, 9), dtype=np.float32)
    img = rng.standard_normal((2, 3, 37, 53), dtype=np.float32)
    stem_w = (rng.standard_normal((64, 3, 3, 3)) / 5).astype(np.float32)
    pa, ua, xa = window_act(K, px), window_act(K, ux), window_act(K, x)
    imgd, swd = dev(img), dev(stem_w)
    sizes = [g[f"up_{t}_y"].shape[2:] for t in "abc"]
    gys = [window_act(K, g[f"up_{t}_gy"]) for t in "abc"]
    c70 = rng.standard_normal((1, 70, 9, 13), dtype=np.float32)
    c70d = dev(c70)
    wst = torch.nn.Parameter(swd.clone())

    def run():
        drop_packs(wst)
        outs = [K.maxpool3s2(pa).nchw(), K.gap(xa), K.colsum(xa)]
        for (oh, ow), gy in zip(sizes, gys):
            outs += [K.upsample_ac(ua, int(oh), int(ow)).nchw(), K.upsample_ac_bwd(gy, ux.shape[2], ux.shape[3]).nchw()]
        outs.append(K.stem_conv_pool(imgd, swd).nchw())
        sa = K.stem_im2col(imgd)
        outs.append(K.conv2d(sa, K.packed_stem(wst)).nchw())
        na = K.nchw_to_act(c70d)
        outs.append(na.buf)
        return outs

    r_ = poison_runs(run)
    conv = f64_conv(img, stem_w, 1, 1, 1)
    pooled = torch.nn.functional.max_pool2d(torch.from_numpy(conv), 3, 2, 1).numpy()
    for o in each_run(r_):
        np.testing.assert_array_equal(o[0].numpy(), g["pool_y"])
        close(o[1], x.mean((2, 3)), 1e-5, 1e-6)
        close(o[2], x.sum((2, 3)), 1e-5, 1e-4)
        for i, t in enumerate("abc"):
            close(o[3 + 2 * i], g[f"up_{t}_y"], 1e-5, 5e-6)
            close(o[4 + 2 * i], g[f"up_{t}_gx"], 1e-4, 1e-5)
        close(o[9], pooled, 1e-4, 1e-4)
        close(o[10], conv, 1e-4, 1e-4)
        np.testing.assert_array_equal(o[11][..., :70].permute(0, 3, 1, 2).numpy(), c70)
        assert (o[11][..., 70:] == 0).all()


def test_gap_from_partials(K):
    """gap() from the conv epilogue's partial sums (x.stats) instead of a pass over the map."""
    torch.manual_seed(1)
    x = K.Act(torch.randn(2, 8, 8, 256, device="cuda"))
    wt = torch.randn(512, 256, 1, 1, device="cuda") / 16

    def run():
        y = K.conv2d(x, K.pack_weight(wt), want_stats=True)
        return [K.gap(y), y.nchw()]

    r_ = poison_runs(run)
    ref = torch.nn.functional.conv2d(x.nchw().double(), wt.double()).cpu()
    for o in each_run(r_):
        close(o[0], ref.mean((2, 3)).numpy(), 1e-5, 1e-5)


def test_groupnorm_layernorm_upsample_bilinear(K):
    """GroupNorm (+ReLU) forward / backward with its workspaces, residual + LayerNorm forward / backward, half-pixel bilinear
    + add, NHWC -> NCHW; vs float64 autograd."""
    from multishiftseg_amd._lib import ptr
    rng = np.random.default_rng(7)
    n, c, h, w = 2, 256, 11, 13
    x = rng.standard_normal((n, c, h, w), dtype=np.float32) * 2 + 1
    gy = rng.standard_normal((n, c, h, w), dtype=np.float32)
    gn = torch.nn.GroupNorm(32, c)
    with torch.no_grad():
        gn.weight.uniform_(0.5, 1.5)
        gn.bias.normal_()
    xd = torch.from_numpy(x).double().requires_grad_(True)
    gnd = torch.nn.GroupNorm(32, c).double()
    gnd.load_state_dict(gn.state_dict())
    torch.relu(gnd(xd)).backward(torch.from_numpy(gy).double())
    y_ref = torch.relu(gnd(torch.from_numpy(x).double())).detach().numpy()
    gn = gn.cuda()
    xa, ga = window_act(K, x, c0=0, extra=0), window_act(K, gy, c0=0, extra=0)
    ln = torch.nn.LayerNorm(c).cuda()
    with torch.no_grad():
        ln.weight.uniform_(0.5, 1.5)
        ln.bias.normal_()
    a = torch.randn(3, 77, c, device="cuda")
    b = torch.randn(3, 77, c, device="cuda")
    gl = torch.randn(3, 77, c, device="cuda")
    top = window_act(K, rng.standard_normal((n, c, 5, 6), dtype=np.float32), c0=0, extra=0)

    def run():
        y, stat = K.groupnorm(xa, gn, relu=True, want_stat=True)
        dx, dg, db = K.groupnorm_backward(ga.ptr, ga.ld, ga.H * ga.W * ga.ld, xa, gn, stat, relu=True)
        aa, bb = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        z = K.add_layernorm(aa, bb, ln)
        ln.weight.grad = ln.bias.grad = None
        z.backward(gl)
        up = K.upsample_bilinear_add(top, xa)
        return [y.nchw(), dx.nchw(), dg, db, z, aa.grad, bb.grad, ln.weight.grad, ln.bias.grad, K.nhwc_to_nchw(up)]

    r_ = poison_runs(run)
    ad, bd = a.double().cpu().requires_grad_(True), b.double().cpu().requires_grad_(True)
    lnd = torch.nn.LayerNorm(c).double()
    lnd.load_state_dict({k: v.cpu() for k, v in ln.state_dict().items()})
    zd = lnd(ad + bd)
    zd.backward(gl.double().cpu())
    upd = torch.from_numpy(x).double() + torch.nn.functional.interpolate(top.nchw().double().cpu(), size=(h, w), mode="bilinear",
                                                                         align_corners=False)
    for o in each_run(r_):
        close(o[0], y_ref, 1e-4, 1e-4)
        close(o[1], xd.grad.numpy(), 1e-4, 1e-4)
        close(o[2], gnd.weight.grad.numpy(), 1e-4, 1e-4)
        close(o[3], gnd.bias.grad.numpy(), 1e-4, 1e-4)
        close(o[4], zd.detach().numpy(), 1e-4, 1e-4)
        close(o[5], ad.grad.numpy(), 1e-4, 1e-4)
        close(o[6], ad.grad.numpy(), 1e-4, 1e-4)
        close(o[7], lnd.weight.grad.numpy(), 1e-4, 1e-3)
        close(o[8], lnd.bias.grad.numpy(), 1e-4, 1e-3)
        close(o[9], upd.numpy(), 1e-5, 1e-5)


# ---- heads and Linears ------------------------------------------------------------------------------------------------------
def test_linear_and_ffn(K, gemm_route):
    """linear (+ReLU) and the FFN node forward / backward on the MFMA kernels: outputs and every gradient vs float64."""
    from multishiftseg_amd import linear as L
    torch.manual_seed(3)
    x = torch.randn(2, 333, 256, device="cuda")
    lin1, lin2 = torch.nn.Linear(256, 1024).cuda(), torch.nn.Linear(1024, 256).cuda()
    lin3 = torch.nn.Linear(256, 80).cuda()
    gy = torch.randn(2, 333, 256, device="cuda")
    g3 = torch.randn(2, 333, 80, device="cuda")
    params = list(lin1.parameters()) + list(lin2.parameters()) + list(lin3.parameters())

    def run():
        drop_packs(*params)
        for p in params:
            p.grad = None
        xx = x.clone().requires_grad_(True)
        y = L.ffn_relu(xx, lin1, lin2)
        z = L.linear(xx, lin3.weight, lin3.bias, relu=True)
        torch.autograd.backward([y, z], [gy, g3])
        return [y, z, xx.grad] + [p.grad for p in params]

    r_ = poison_runs(run)
    xd = x.double().cpu().requires_grad_(True)
    pd = [p.detach().double().cpu().requires_grad_(True) for p in params]
    yd = torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(xd, pd[0], pd[1])), pd[2], pd[3])
    zd = torch.relu(torch.nn.functional.linear(xd, pd[4], pd[5]))
    torch.autograd.backward([yd, zd], [gy.double().cpu(), g3.double().cpu()])
    wants = [yd.detach(), zd.detach(), xd.grad] + [p.grad for p in pd]
    for o in each_run(r_):
        for i, (got, want) in enumerate(zip(o, wants)):
            s = float(want.abs().max())
            assert (got.double() - want).abs().max().item() <= 1e-5 * s + 1e-5, i


def test_ood_tail_and_m2f_scores(K):
    """The OOD tail (score, logits, labels) from head slices of a 48-channel map and its backward; the M2F score unfused and
    fused (mask logits GEMM + upsample + class mix); vs float64 / the reference's vectors."""
    rng = np.random.default_rng(6)
    n, h, w = 2, 13, 18
    d = rng.standard_normal((n, 48, h, w), dtype=np.float32) * 3
    da = window_act(K, d, c0=0, extra=0)
    oh, ow = 26, 36
    dt = torch.from_numpy(d).double().requires_grad_(True)
    lg = torch.nn.functional.interpolate(dt[:, 0:19], size=(oh, ow), mode="bilinear", align_corners=True)
    sc = torch.nn.functional.interpolate(-torch.logsumexp(dt[:, 20:39], 1, keepdim=True), size=(oh, ow), mode="bilinear",
                                         align_corners=True)[:, 0]
    gl = rng.standard_normal(tuple(lg.shape), dtype=np.float32)
    gs = rng.standard_normal(tuple(sc.shape), dtype=np.float32)
    ((lg * torch.from_numpy(gl).double()).sum() + (sc * torch.from_numpy(gs).double()).sum()).backward()
    gsd, gld = dev(gs), dev(gl)
    g = golden("m2f_score")
    size = tuple(int(v) for v in g["size"])
    clsd, maskd = dev(g["cls"]), dev(g["mask"])
    gf = golden("m2f_fused")
    tag = "ragged"
    image, crop = tuple(int(v) for v in gf[tag + "_image"]), tuple(int(v) for v in gf[tag + "_crop"])
    emb, feat, cls2 = dev(gf[tag + "_embed"]), dev(gf[tag + "_features"]), dev(gf[tag + "_cls"])

    def run():
        s, l, lab = K.ood_score(da.slice(20, 19), da.slice(0, 19), oh, ow, want_label=True)
        dd = K.Act.empty(n, h, w, 48, "cuda")
        dd.buf.zero_()
        K.ood_score_bwd(da.slice(20, 19), gsd, gld, dd.slice(20, 19), dd.slice(0, 19), oh, ow)
        m = K.m2f_mask_logits(emb, feat)
        return [s, l, lab, dd.nchw(), K.m2f_score(clsd, maskd, size), K.m2f_score_fused(cls2, m, image, crop)]

    r_ = poison_runs(run)
    for o in each_run(r_):
        close(o[0], sc.detach().numpy(), 1e-5, 1e-5)
        close(o[1], lg.detach().numpy(), 1e-5, 1e-5)
        np.testing.assert_array_equal(o[2].numpy(), o[1].numpy().argmax(1))
        close(o[3], dt.grad.numpy(), 1e-4, 1e-5)
        close(o[4], g["score"], 1e-5, 1e-5)
        close(o[5], gf[tag + "_score"], 1e-5, 1e-5)


# ---- MSDeformAttn ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["0", "b"])
def test_msda_core_both_backward_formulations(monkeypatch, mode):
    """The sampling op forward and both grad_value formulations (generic scatter-add, binned owner-computes) with grad_value,
    grad_loc, grad_attn and the binned workspace from torch.empty; vs the float64 oracle (test_backward_formulations_vs_oracle)."""
    from multishiftseg_amd import MultiScaleDeformableAttention as MSDA
    monkeypatch.setenv("MSS_MSDA_BWD_BINNED", "1" if mode == "b" else "0")
    rng = np.random.default_rng(9)
    shp = np.array([(12, 20), (7, 9), (3, 5)], dtype=np.int64)
    starts = np.concatenate([[0], np.cumsum(shp.prod(1))[:-1]]).astype(np.int64)
    S, L, N, Lq = int(shp.prod(1).sum()), 3, 2, 333
    value = rng.standard_normal((N, S, 8, 32), dtype=np.float32)
    loc = rng.uniform(-0.2, 1.2, (N, Lq, 8, L, 4, 2)).astype(np.float32)
    attn = rng.random((N, Lq, 8, L, 4), dtype=np.float32)
    attn /= attn.sum((-1, -2), keepdims=True)
    gout = rng.standard_normal((N, Lq, 256), dtype=np.float32)
    args = [dev(value), dev(shp), dev(starts), dev(loc), dev(attn)]
    god = dev(gout)

    def run():
        out = MSDA.ms_deform_attn_forward(*args, 2)
        return [out] + MSDA.ms_deform_attn_backward(*args, god, 2)

    r_ = poison_runs(run)
    ro = omsda.forward(value, shp, starts, loc, attn)
    gv, gl, ga = omsda.backward(value, shp, starts, loc, attn, gout)
    for o in each_run(r_):
        close(o[0], ro, 1e-4, 1e-5)
        close(o[1], gv, 1e-3, 1e-4)
        close(o[2], gl, 1e-3, 3e-3)
        close(o[3], ga, 1e-3, 1e-4)


def test_msda_module_prepare_sample_backward(gemm_route):
    """MSDeformAttn module (prepare: softmax + locations, fused sample, the projected backward) forward and backward: the poisoned
    runs equal the clean one bit for bit and are finite (the module's agreement with float64 is tests/test_gpu_msda.py's; the
    sampling op under poison is held to the float64 oracle above)."""
    from multishiftseg_amd.ms_deform_attn import MSDeformAttn
    torch.manual_seed(4)
    m = MSDeformAttn(256, 3, 8, 4).cuda()
    with torch.no_grad():
        m.sampling_offsets.weight.normal_(0, 0.02)
        m.attention_weights.weight.normal_(0, 0.02)
    shp = torch.tensor([(12, 20), (7, 9), (3, 5)], device="cuda")
    starts = torch.tensor([0, 240, 303], device="cuda")
    S = 318
    q = torch.randn(2, S, 256, device="cuda")
    src = torch.randn(2, S, 256, device="cuda")
    ref = torch.rand(2, S, 3, 2, device="cuda")
    gy = torch.randn(2, S, 256, device="cuda")
    params = list(m.parameters())

    def run():
        drop_packs(*params)
        for p in params:
            p.grad = None
        qq, ss = q.clone().requires_grad_(True), src.clone().requires_grad_(True)
        y = m(qq, ref, ss, shp, starts)
        y.backward(gy)
        return [y, qq.grad, ss.grad] + [p.grad for p in params]

    r_ = poison_runs(run, bitwise=True)
    for o in each_run(r_):
        assert all(bool(torch.isfinite(t).all()) for t in o)


# ---- loss, metric, optimizer --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["deeplab_4x32x32", "m2f_4x32x32", "ratio1_4x16x16", "no_ood_4x16x16", "no_in_aug_4x16x16",
                                 "deeplab_8x48x40"])
def test_loss_fixtures(tag):
    """RelContrastiveLoss (reference pairing, the reference's permutations injected) on the rcl_* fixtures at test_golden's
    bounds. The loss sums its counters with float64 atomics: the loss value is held to the fixture bound, not bitwise."""
    from multishiftseg_amd.loss import RelContrastiveLoss
    g = golden("rcl_" + tag)
    params = ast.literal_eval(str(g["params"]))
    B, C, H, W = (int(v) for v in g["shape"])
    logits = g["logits"] if g["logits"].size else \
        np.random.default_rng(int(g["seed"])).standard_normal((B, C, H, W), dtype=np.float32) * 3
    perms = [torch.from_numpy(g[f"perm{i}"].astype(np.int64)) for i in range(3)]
    ld, sd, td = dev(logits), dev(g["score"]), dev(g["target"].astype(np.int64))

    def run():
        crit = RelContrastiveLoss(params)
        lt, st, tt = ld.clone().requires_grad_(True), sd.clone().requires_grad_(True), td.clone()
        loss = crit(lt, st, tt, perms=perms)
        if torch.isfinite(loss):
            loss.backward()
        return [loss, lt.grad, st.grad, crit.last_terms, tt]

    nan_loss = np.isnan(g["loss"])
    r_ = poison_runs(run, allow_nonfinite=nan_loss)
    for o in each_run(r_):
        np.testing.assert_array_equal(o[-1].numpy().astype(np.uint8), g["target_mut"])
        if nan_loss:
            assert torch.isnan(o[0])
            continue
        np.testing.assert_allclose(o[0].item(), g["loss"], rtol=1e-5)
        close(o[2], g["dscore"], 1e-4, 1e-8)
        d = o[1].numpy()
        if "dlogit" in g:
            close(d, g["dlogit"], 1e-3, 1e-7)
        else:
            close(d[:, :, ::3, ::3], g["dlogit_sub"], 1e-3, 1e-7)
        np.testing.assert_allclose(np.abs(d.astype(np.float64)).sum(), g["dlogit_abs_sum"], rtol=1e-4)


def test_loss_device_pairing():
    """The one-call device-pairing loss (one byte workspace, dlogit / dscore / out from torch.empty) under poison: against the
    reference-pairing run of the same inputs for the pairing-free terms (CE parts), finite everywhere."""
    from multishiftseg_amd.loss import RelContrastiveLoss
    from multishiftseg_amd.trainer import LOSS_PARAMS
    g = golden("rcl_deeplab_8x48x40")
    B, C, H, W = (int(v) for v in g["shape"])
    logits = np.random.default_rng(int(g["seed"])).standard_normal((B, C, H, W), dtype=np.float32) * 3 \
        if not g["logits"].size else g["logits"]
    ld, sd, td = dev(logits), dev(g["score"]), dev(g["target"].astype(np.int64))

    def run():
        crit = RelContrastiveLoss(LOSS_PARAMS, pairing="device", seed=3)
        lt, st, tt = ld.clone().requires_grad_(True), sd.clone().requires_grad_(True), td.clone()
        loss = crit(lt, st, tt)
        loss.backward()
        return [loss, lt.grad, st.grad, crit.last_terms, tt]

    r_ = poison_runs(run)
    clean = r_["clean"]
    for o in each_run(r_):
        assert torch.isfinite(o[0]) and abs(o[0].item() - clean[0].item()) <= 1e-5 * abs(clean[0].item())
        np.testing.assert_allclose(o[1].numpy(), clean[1].numpy(), rtol=1e-5, atol=1e-9)
        np.testing.assert_allclose(o[2].numpy(), clean[2].numpy(), rtol=1e-5, atol=1e-9)
        np.testing.assert_array_equal(o[4].numpy(), clean[4].numpy())


def test_metric_fixture_update_many_compute():
    """OOD measures on the ood_metrics fixture (eval_ood_measure) and the streamed meter (update, update_many, compute) at
    test_golden_reference_measures' tolerance."""
    from multishiftseg_amd import metric as M
    g = golden("ood_metrics")
    tags = sorted(k[:-len("_measures")] for k in g.files if k.endswith("_measures"))
    data = [(dev(g[t + "_score"]), dev(g[t + "_label"].astype(np.int64))) for t in tags]

    def run():
        outs = [torch.from_numpy(np.asarray(M.eval_ood_measure(s, l), dtype=np.float64)) for s, l in data]
        a, b = M.OODMeter(), M.OODMeter()
        for s, l in data[:1]:
            a.update(s, l)
        b.update_many(data[:1])
        outs += [torch.from_numpy(np.asarray(r, dtype=np.float64)) for r in (a.compute(), b.compute())]
        return outs

    r_ = poison_runs(run, bitwise=True)
    for o in each_run(r_):
        for t, got in zip(tags, o):
            np.testing.assert_allclose(got.numpy(), g[t + "_measures"], rtol=0, atol=1e-11, err_msg=t)
        np.testing.assert_allclose(o[-2].numpy(), g[tags[0] + "_measures"], rtol=0, atol=1e-11)
        np.testing.assert_array_equal(o[-1].numpy(), o[-2].numpy())


def test_adam_step():
    """The HIP Adam on fresh state (torch.zeros_like moments) against float64 torch.optim.Adam arithmetic."""
    from multishiftseg_amd.optim import Adam
    torch.manual_seed(2)
    p0 = torch.randn(1000, 37, device="cuda")
    gr = torch.randn(1000, 37, device="cuda")

    def run():
        p = torch.nn.Parameter(p0.clone())
        p.grad = gr.clone()
        opt = Adam([p], lr=1e-3, weight_decay=1e-4)
        opt.step()
        opt.step()
        return [p.detach()]

    r_ = poison_runs(run, bitwise=True)
    pd = torch.nn.Parameter(p0.double().cpu())
    pd.grad = gr.double().cpu()
    ref = torch.optim.Adam([pd], lr=1e-3, weight_decay=1e-4)
    ref.step()
    ref.step()
    for o in each_run(r_):
        assert (o[0].double() - pd.detach()).abs().max().item() < 1e-6


# ---- whole paths against the reference's fixtures --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def deeplab(deeplab_params):
    from multishiftseg_amd.deepv3 import DeepWV3Plus
    m = DeepWV3Plus(19)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in deeplab_params.items()}, strict=True)
    return m.cuda()


def test_deeplab_eval_fixture(deeplab, gemm_route):
    """DeepLab eval forward on deepwv3plus_eval_2x96x96, every packed weight made inside the poison: bit for bit the clean run
    (the forward is bit-reproducible), and the fixture's 1e-3 bound."""
    from multishiftseg_amd import synth
    g = golden("deepwv3plus_eval_2x96x96")
    n, h, w = (int(v) for v in g["shape"])
    img = torch.from_numpy(synth.synth_image(int(g["image_seed"]), n, h, w)).cuda()
    deeplab.eval()

    def run():
        drop_packs(*deeplab.parameters())
        with torch.no_grad():
            return list(deeplab(img))

    r_ = poison_runs(run, bitwise=True)
    for o in each_run(r_):
        assert np.abs(o[1].numpy() - g["logit"]).max() < 1e-3
        assert np.abs(o[0].numpy() - g["score"]).max() < 1e-3


@pytest.mark.parametrize("n,h,w,train", [(1, 90, 150, False), (2, 70, 70, True)])
def test_deeplab_ragged_sizes_vs_oracle(deeplab, deeplab_params, n, h, w, train, gemm_route):
    """The ragged sizes of test_forward_vs_oracle_ragged_sizes under poison: bit for bit the clean run, 1e-3 of the oracle."""
    from multishiftseg_amd import synth
    from oracle import deepv3 as odeepv3
    img = synth.synth_image(11, n, h, w)
    imgd = torch.from_numpy(img).cuda()
    rng = np.random.default_rng(5)
    masks = None
    saved = {k: v.detach().clone() for k, v in deeplab.state_dict().items()}
    if train:
        masks = {"mod6": ((rng.random((n, 1024)) >= 0.3) / 0.7).astype(np.float32),
                 "mod7": ((rng.random((n, 2048)) >= 0.5) / 0.5).astype(np.float32)}

    def setup():
        deeplab.load_state_dict(saved)
        if train:
            deeplab.train()
            deeplab.dropout_masks = {k: torch.from_numpy(v) for k, v in masks.items()}
        else:
            deeplab.eval()

    def run():
        drop_packs(*deeplab.parameters())
        with torch.no_grad():
            return list(deeplab(imgd)) + ([deeplab.final[1].running_mean.clone()] if train else [])

    try:
        r_ = poison_runs(run, setup=setup, bitwise=True)
    finally:
        deeplab.dropout_masks = None
        deeplab.load_state_dict(saved)
        deeplab.eval()
    rs, rl = odeepv3.forward(deeplab_params, img, train=train, drop_masks=masks)
    for o in each_run(r_):
        assert np.abs(o[1].numpy() - rl).max() < 1e-3
        assert np.abs(o[0].numpy() - rs).max() < 1e-3


@pytest.mark.parametrize("stage", [1, 2])
def test_train_step_fixture(deeplab_params, stage, gemm_route):
    """One TrainStep (forward with train-mode BN, fused loss, backward, HIP Adam) on deepwv3plus_train_step with the reference's
    dropout masks and permutations injected. The loss sums counters with float64 atomics, so the loss value and everything
    downstream of it (gradients, updated weights) is compared bitwise only where two clean runs agree bitwise and is otherwise
    held to the fixture bounds (score / logits 1e-3, loss rtol 1e-4); score and logits precede the loss and are bitwise."""
    from multishiftseg_amd import synth
    from multishiftseg_amd.deepv3 import DeepWV3Plus
    from multishiftseg_amd.loss import RelContrastiveLoss
    from multishiftseg_amd.trainer import LOSS_PARAMS, TrainStep
    g = golden("deepwv3plus_train_step")
    pairs, h, w = (int(v) for v in g["shape"])
    m = DeepWV3Plus(19)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in deeplab_params.items()}, strict=True)
    m = m.cuda()
    m.uncertainty_func_init()
    saved = {k: v.detach().clone() for k, v in m.state_dict().items()}
    pre = f"stage{stage}_"
    img = torch.from_numpy(synth.synth_image(int(g["image_seed"]), 2 * pairs, h, w)).cuda()
    target = torch.from_numpy(g["target"].astype(np.int64)).cuda()
    perms = [torch.from_numpy(g[pre + f"perm{i}"].astype(np.int64)) for i in range(3)]
    masks = {"mod6": torch.from_numpy(g[pre + "drop_mod6"]), "mod7": torch.from_numpy(g[pre + "drop_mod7"])}

    def setup():
        m.load_state_dict(saved)
        for p in m.parameters():
            p.grad = None

    def run():
        drop_packs(*m.parameters())
        step = TrainStep(m, RelContrastiveLoss(LOSS_PARAMS), stage=stage)
        step.keep_outputs = True
        m.dropout_masks = dict(masks)
        loss = step(img, target.clone(), perms=perms)
        score, logit = step.last_outputs
        names = sorted(step.names)
        pd = dict(m.named_parameters())
        return [score.detach(), logit.detach(), loss.detach()] + [pd[k].grad for k in names] + [pd[k].detach() for k in names]

    r_ = poison_runs(run, setup=setup)
    assert r_["reproducible"][0] and r_["reproducible"][1], "score / logits of two clean runs differ"
    for o in each_run(r_):
        close(o[0], g[pre + "score"], 0, 1e-3)
        close(o[1][:, :, ::4, ::4], g[pre + "logit_sub"], 0, 1e-3)
        np.testing.assert_allclose(o[2].item(), float(g[pre + "loss"]), rtol=1e-4)
        for i, t in enumerate(o[3:]):
            assert torch.isfinite(t).all(), i


def test_m2f_decoder_fixture_forward_backward(gemm_route):
    """M2F pixel decoder forward and backward on m2f_decoder (test_decoder_forward_features_golden's 1e-3 bounds, gradient L2
    norms within 1e-3 of the reference's); the decoder is bit-reproducible, so poisoned runs equal the clean one bit for bit."""
    from test_decoder import SHAPE, build
    dec, g = build()
    dec = dec.cuda()
    rng = np.random.default_rng(int(g["seed"]))
    H, W = (int(v) for v in g["hw"])
    feats_np = {k: rng.standard_normal((2, c, H // s, W // s), dtype=np.float32) for k, (c, s) in SHAPE.items()}
    crng = np.random.default_rng(int(g["cot_seed"]))
    shapes = [(2, 256, 24, 40), (2, 256, 3, 5), (2, 256, 6, 10), (2, 256, 12, 20)]
    cot = [torch.from_numpy(crng.standard_normal(s, dtype=np.float32)).cuda() for s in shapes]
    feats_d = {k: dev(v) for k, v in feats_np.items()}
    names = [k for k, _ in dec.named_parameters()]

    def run():
        drop_packs(*dec.parameters())
        for p in dec.parameters():
            p.requires_grad_(True)
            p.grad = None
        feats = {k: v.clone().requires_grad_(True) for k, v in feats_d.items()}
        mask, out0, ms = dec.forward_features(feats)
        sum((t * c).sum() for t, c in zip((mask, *ms), cot)).backward()
        pd = dict(dec.named_parameters())
        return [mask.detach(), ms[0].detach(), ms[1].detach(), ms[2].detach()] + [pd[k].grad for k in names] + \
            [feats[k].grad for k in sorted(feats)]

    r_ = poison_runs(run, bitwise=True)
    for o in each_run(r_):
        close(o[0][:, ::4], g["mask_sub"], 1e-3, 1e-3)
        close(o[1], g["out0"], 1e-3, 1e-3)
        close(o[2][:, ::2], g["ms1"], 1e-3, 1e-3)
        close(o[3][:, ::4], g["ms2_sub"], 1e-3, 1e-3)
        for k, gr in zip(names, o[4:4 + len(names)]):
            np.testing.assert_allclose(gr.double().norm().item(), float(g["gl2_" + k]), rtol=1e-3, err_msg=k)
        for k, gr in zip(sorted(feats_np), o[4 + len(names):]):
            np.testing.assert_allclose(gr.double().norm().item(), float(g["gl2_feat_" + k]), rtol=1e-3, err_msg=k)
