"""The class-generic route of the OOD-score tail (csrc/glue.hip), alone: forward against oracle.nnops.ood_score_tail, backward
against torch autograd of the same composition, with the bounds tests/test_gpu_ops.py::test_ood_score_tail uses at 19 classes
(forward rtol 1e-5 / atol 1e-5, backward rtol 1e-4 / atol 1e-5; the label bit-equal to the argmax of the kernel's own logits).
Both heads live in one pixel-contiguous buffer laid out by deepv3.heads_layout, as the model hands them over."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import nnops

pytestmark = pytest.mark.gpu

# the kernel's chunk constant, read from the source so that the chunk edges below follow it
CH = int(re.search(r"constexpr int OOD_CH = (\d+);", open(os.path.join(ROOT, "multishiftseg_amd", "csrc", "glue.hip")).read()).group(1))
CLASSES = sorted({1, 2, 3, 4, 5, 12, 100, CH - 1, CH, CH + 1, 2 * CH + 1})
N = 2
# (source, output): the smallest shapes that reach every regime and a ragged second tile in both directions
SHAPES = {
    "vector": ((13, 18), (26, 36)),             # OW % 4 == 0, aligned, x2
    "ow_mod4": ((13, 17), (26, 34)),            # OW % 4 != 0: tiled forward, per-pixel backward
    "odd": ((13, 17), (25, 33)),
    "identity": ((13, 17), (13, 17)),
    "down": ((13, 17), (7, 9)),                 # down-sampling: per-pixel fallback
    "two_tiles": ((9, 70), (18, 140)),          # two tiles in x and in y, forward (8 x 128) and backward (4 x 64)
}


@pytest.fixture(scope="module")
def K():
    from multishiftseg_amd import kernels
    return kernels


@pytest.fixture
def generic_route():
    """MSS_OOD_TAIL_GENERIC=1 for one test: C == 19 goes through the generic kernels too."""
    from multishiftseg_amd import _lib
    os.environ["MSS_OOD_TAIL_GENERIC"] = "1"
    _lib.reset_env_cache()
    try:
        yield
    finally:
        del os.environ["MSS_OOD_TAIL_GENERIC"]
        _lib.reset_env_cache()


def heads_buffer(K, d, shift=0):
    """NCHW array [N, Kh, h, w] -> Act over an NHWC device buffer whose first element sits `shift` floats past an aligned one."""
    n, kh, h, w = d.shape
    flat = torch.empty(n * h * w * kh + 4, device="cuda", dtype=torch.float32)
    assert flat.data_ptr() % 16 == 0
    view = flat[shift:shift + n * h * w * kh].view(n, h, w, kh)
    view.copy_(torch.from_numpy(np.ascontiguousarray(d.transpose(0, 2, 3, 1))))
    return K.Act(view)


def nan_buffer(K, n, h, w, kh, shift=0):
    flat = torch.full((n * h * w * kh + 4,), float("nan"), device="cuda", dtype=torch.float32)
    return K.Act(flat[shift:shift + n * h * w * kh].view(n, h, w, kh))


def check_tail(K, C, src, out, seed, shift=0, nan_dest=True):
    from multishiftseg_amd.deepv3 import heads_layout
    q, Kh = heads_layout(C)
    (h, w), (oh, ow) = src, out
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((N, Kh, h, w), dtype=np.float32) * 3
    da = heads_buffer(K, d, shift)
    dec2, dec1 = da.slice(q, C), da.slice(0, C)
    # ---- forward
    score, logit, label = K.ood_score(dec2, dec1, oh, ow, want_label=True)
    assert tuple(logit.shape) == (N, C, oh, ow) and label.dtype == torch.uint8
    rs, rl = nnops.ood_score_tail(d[:, q:q + C], d[:, 0:C], (oh, ow))
    got = logit.cpu().numpy()
    np.testing.assert_allclose(score.cpu().numpy(), rs, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(got, rl, rtol=1e-5, atol=1e-5)
    np.testing.assert_array_equal(label.cpu().numpy(), got.argmax(1))          # bit-exact against its own logits
    # each output alone gives the same bits as all three together
    s1, _, _ = K.ood_score(dec2, None, oh, ow, want_logit=False)
    _, _, l1 = K.ood_score(None, dec1, oh, ow, want_score=False, want_logit=False, want_label=True)
    assert torch.equal(s1, score) and torch.equal(l1, label)
    # ---- backward against autograd of the same composition
    dt = torch.from_numpy(d).requires_grad_(True)
    lg = torch.nn.functional.interpolate(dt[:, 0:C], size=(oh, ow), mode="bilinear", align_corners=True)
    sc = torch.nn.functional.interpolate(-torch.logsumexp(dt[:, q:q + C], 1, keepdim=True), size=(oh, ow), mode="bilinear",
                                         align_corners=True)[:, 0]
    gl = torch.from_numpy(rng.standard_normal(tuple(lg.shape), dtype=np.float32))
    gs = torch.from_numpy(rng.standard_normal(tuple(sc.shape), dtype=np.float32))
    (g1,) = torch.autograd.grad((lg * gl).sum(), dt, retain_graph=True)
    (g2,) = torch.autograd.grad((sc * gs).sum(), dt)
    g1, g2 = g1.numpy(), g2.numpy()
    heads = np.zeros(Kh, dtype=bool)
    heads[0:C] = heads[q:q + C] = True
    for name, dscore, dlogit, want in (("both", gs, gl, g1 + g2), ("dscore", gs, None, g2), ("dlogit", None, gl, g1)):
        dd = nan_buffer(K, N, h, w, Kh, shift) if nan_dest else K.Act.zeros(N, h, w, Kh, "cuda")
        K.ood_score_bwd(dec2, dscore.cuda() if dscore is not None else None, dlogit.cuda() if dlogit is not None else None,
                        dd.slice(q, C), dd.slice(0, C), oh, ow)
        res = dd.nchw().cpu().numpy()
        np.testing.assert_allclose(res[:, heads], want[:, heads], rtol=1e-4, atol=1e-5, err_msg=name)
        assert np.all(res[:, ~heads] == 0), name                                # padding columns: exactly 0, never the NaN fill
        if dscore is None:
            assert np.all(res[:, q:q + C] == 0), name                           # the other head's columns: exactly 0
        if dlogit is None:
            assert np.all(res[:, 0:C] == 0), name


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("C", CLASSES)
def test_generic_tail(K, C, shape):
    """Every class count on every regime; the backward runs into a NaN-filled destination, with both gradients and with each
    alone, and the padding columns and an absent gradient's head come back exactly 0."""
    check_tail(K, C, *SHAPES[shape], seed=1000 * C + len(shape))


@pytest.mark.parametrize("C", [12, 2 * CH + 1])
def test_generic_tail_off_a_16_byte_boundary(K, C):
    """Operands 4 bytes past a 16-byte boundary at the vector regime's shape: the 16-byte regimes must step aside."""
    check_tail(K, C, *SHAPES["vector"], seed=77 + C, shift=1)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_19_classes_on_the_generic_route(K, generic_route, shape):
    """MSS_OOD_TAIL_GENERIC=1: the 19 classes pass the same bounds on the generic kernels."""
    check_tail(K, 19, *SHAPES[shape], seed=19 + len(shape))


def test_19_classes_agree_across_the_two_routes(K):
    """The switch is a cross-check: at the two-tile vector shape the two routes see the same operands and differ by rounding only (the
    label may differ only where the two logits sets order a near-tie differently, so it is compared through the logits)."""
    from multishiftseg_amd import _lib
    from multishiftseg_amd.deepv3 import heads_layout
    q, Kh = heads_layout(19)
    (h, w), (oh, ow) = SHAPES["two_tiles"]
    d = np.random.default_rng(5).standard_normal((N, Kh, h, w), dtype=np.float32) * 3
    da = heads_buffer(K, d)
    s0, l0, _ = K.ood_score(da.slice(q, 19), da.slice(0, 19), oh, ow)
    os.environ["MSS_OOD_TAIL_GENERIC"] = "1"
    _lib.reset_env_cache()
    try:
        s1, l1, _ = K.ood_score(da.slice(q, 19), da.slice(0, 19), oh, ow)
    finally:
        del os.environ["MSS_OOD_TAIL_GENERIC"]
        _lib.reset_env_cache()
    np.testing.assert_allclose(s1.cpu().numpy(), s0.cpu().numpy(), rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(l1.cpu().numpy(), l0.cpu().numpy(), rtol=1e-5, atol=1e-5)


def test_nan_is_maximal_and_the_first_one_wins(K):
    """label: the first maximum wins, a NaN is maximal and the first NaN wins -- also across a chunk boundary."""
    from multishiftseg_amd.deepv3 import heads_layout
    C = 2 * CH + 1
    q, Kh = heads_layout(C)
    # four patterns, each on two neighbouring source rows (a blend with weight 0 still spreads a NaN to its neighbour)
    d = np.zeros((1, Kh, 8, 8), dtype=np.float32)
    d[0, CH + 1, 0:2, :] = 5.0                    # a maximum in the second chunk ...
    d[0, 2 * CH, 0:2, :] = 5.0                    # ... tied by a later class: the first wins
    d[0, 3, 2:4, :] = np.nan
    d[0, CH + 2, 2:4, :] = np.nan                 # the first NaN wins over a later one and over every number
    d[0, 2, 4:6, :] = 1.0
    d[0, CH, 4:6, :] = np.nan                     # a NaN in a later chunk beats an earlier maximum
    da = heads_buffer(K, d)                       # rows 6, 7: all equal, class 0
    # x2 in y (scale exactly 0.5: output row 2r blends source rows r and r + 1), constant along x: vector regime, tiled regime, and
    # the identity on the per-pixel fallback
    for oh, ow, step in ((15, 16, 4), (15, 15, 4), (8, 8, 2)):
        _, _, label = K.ood_score(None, da.slice(0, C), oh, ow, want_score=False, want_logit=False, want_label=True)
        lab = label.cpu().numpy()[0, ::step]
        assert (lab[0] == CH + 1).all() and (lab[1] == 3).all() and (lab[2] == CH).all() and (lab[3] == 0).all(), (ow, lab)
