"""GPU: the device code of Mask2Former stage 1 -- the bilinear upsample without a lateral (csrc/norm.hip, lat == NULL), the class-mix
backward without the mask gradient (csrc/m2f_mix.hip, dmasks == NULL), kernels.m2f_semantic_inference and its autograd node --
against the float64 restatement of tests/ref_stage1.py.

Bounds: the rule of tests/test_gpu_class_mix.py (`held`): max|hip - float64| of every output and gradient tensor is at most 8 x
its own floor, floor = max|float32 restatement - float64| on the same inputs (asserted > 0). Where the two variants only leave
work out, the check is torch.equal with the full call.

Conditions on the inputs (conditions, not tolerances): -max_c is discontinuous where two classes tie, so the inputs are those of
tests/test_gpu_class_mix.py (queries that belong to a class, masks that favour it in bands of rows) and each case's seed is
chosen, on a CPU with the restatement alone, such that in float64 the smallest gap between the two largest class maps over ALL
pixels of the crop is at least 64 x the float32 floor of those maps (ref_class_mix.top_gap; asserted by every test that
compares a score or its gradient). Low resolution 5 x 7 -> padded image 20 x 28 -> crop 18 x 27, three images."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_class_mix as ref_mix
import ref_stage1 as ref
from multishiftseg_amd import kernels as K
from test_gpu_class_mix import assert_gap, held, make_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"

B, HW, IMAGE, CROP = 3, (5, 7), (20, 28), (18, 27)
CASES = {
    "q7_c3_ldq8": dict(Q=7, C=3, ldq=8, seed=1),             # odd Q, one NaN pad column, CP = 8
    "q100_c19_ldq100": dict(Q=100, C=19, ldq=100, seed=1),   # the reference's sizes: no pad column, CP = 20
}


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(name):
    cfg = CASES[name]
    c = Case()
    c.Q, c.C, c.ldq = cfg["Q"], cfg["C"], cfg["ldq"]
    rng = np.random.default_rng(7000 + cfg["seed"])
    c.cls, c.x = make_inputs(rng, B, c.Q, c.C, *HW)
    c.cls_ood, _ = make_inputs(rng, B, c.Q, c.C, *HW)
    c.g = rng.standard_normal((B,) + CROP).astype(np.float32)
    return c


@functools.lru_cache(maxsize=None)
def _restated(name, dtype):
    c = _case(name)
    t = lambda a: torch.from_numpy(a).to(dtype)
    cls_ood = t(c.cls_ood).requires_grad_(True)
    o = dict(sem_seg=ref.sem_seg(t(c.cls), t(c.x), IMAGE, CROP), full=ref.class_maps(cls_ood, t(c.x), IMAGE, CROP))
    o["ood_score"] = 1 - ref_mix.first_max(o["full"])
    o["dcls_ood"], = torch.autograd.grad(o["ood_score"], cls_ood, t(c.g))
    return {k: v.detach().double() for k, v in o.items()}


def _pixel_major(m, ldq, pad=float("nan")):
    """NCHW [B,Q,h,w] -> [B,h,w,ldq]; the padding of the query axis holds NaN: the mix kernels never read it."""
    b, q, h, w = m.shape
    out = torch.full((b, h, w, ldq), pad, device=m.device)
    out[..., :q] = m.permute(0, 2, 3, 1)
    return out


def _run(name, images_per_chunk, grad=True):
    c = _case(name)
    d = lambda a: torch.from_numpy(a).to(DEV)
    cls_ood = d(c.cls_ood).requires_grad_(grad)
    lg = _pixel_major(d(c.x), c.ldq)
    budget = images_per_chunk * IMAGE[0] * IMAGE[1] * c.ldq * 4
    assert [n for _, n in K.stage1_chunks(B, *IMAGE, c.ldq, budget)] == {1: [1, 1, 1], 2: [2, 1], 3: [3]}[images_per_chunk]
    sem, score = K.m2f_semantic_inference(d(c.cls), lg, IMAGE, CROP, class_logits_ood=cls_ood, Q=c.Q, budget=budget)
    o = dict(sem_seg=sem, ood_score=score.detach())
    if grad:
        assert sem.requires_grad is False and score.requires_grad
        score.backward(d(c.g))
        o["dcls_ood"] = cls_ood.grad
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


@functools.lru_cache(maxsize=None)
def _first_run(name):
    return _run(name, 3)


# ---- the upsample with lat == NULL ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 5, 7, 8), (1, 5, 7, 100)])         # the second: several workgroups per output row
def test_upsample_without_a_lateral(shape):
    x = torch.from_numpy(np.random.default_rng(11).standard_normal(shape).astype(np.float32))
    got = K.upsample_bilinear_nhwc(x.to(DEV), IMAGE)
    n, _, _, ch = shape
    zero_lat = K.Act(torch.zeros((n,) + IMAGE + (ch,), device=DEV))
    add_form = K.upsample_bilinear_add(K.Act(x.to(DEV).contiguous()), zero_lat)
    assert tuple(got.shape) == (n,) + IMAGE + (ch,)
    assert torch.equal(got, add_form.buf)
    want = {dt: F.interpolate(x.to(dt).permute(0, 3, 1, 2), size=IMAGE, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
            for dt in (torch.float64, torch.float32)}
    held(f"upsample {shape}", got.cpu(), want[torch.float64], want[torch.float32].double())


def test_upsample_without_a_lateral_ignores_ldl():
    """lat == NULL with an ldl that the add form refuses: the entry point neither reads nor checks it."""
    from multishiftseg_amd import _lib as L
    x = torch.randn((1, 5, 7, 8), device=DEV)
    y = torch.empty((1,) + IMAGE + (8,), device=DEV)
    L.call("mss_upsample_bilinear_add_nhwc_f32", L.ptr(x), 8, 5 * 7 * 8, 1, 5, 7, None, 7, L.ptr(y), 8, IMAGE[0], IMAGE[1], 8)
    assert torch.equal(y, K.upsample_bilinear_nhwc(x, IMAGE))


# ---- the mix backward with dmasks == NULL -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q,C,ldq", [(7, 3, 8), (100, 19, 104)])
def test_mix_backward_without_dmasks_gives_the_bits_of_the_full_call(Q, C, ldq):
    rng = np.random.default_rng(13)
    h, w = 20, 28                                                   # 560 pixels: one full 512-pixel partial sum and a ragged one
    assert K._lib.value("mss_m2f_mix_backward_chunks", h * w) == 2
    cls, x = make_inputs(rng, 2, Q, C, h, w)
    cls, x = torch.from_numpy(cls).to(DEV), torch.from_numpy(x).to(DEV)
    dmix = torch.from_numpy(rng.standard_normal((2, C, h, w)).astype(np.float32)).to(DEV)
    got = {}
    for pm in (False, True):
        xl = _pixel_major(x, ldq) if pm else x
        _, prob = K.m2f_class_mix(cls, xl, pixel_major=pm, Q=Q)
        dx, full = K.m2f_class_mix_backward(dmix, prob, cls, xl, pixel_major=pm, Q=Q)
        none, alone = K.m2f_class_mix_backward(dmix, prob, cls, xl, pixel_major=pm, Q=Q, want_dmasks=False)
        assert none is None and dx is not None
        assert torch.isfinite(alone).all() and bool((alone != 0).any())
        assert torch.equal(alone, full), f"pixel_major={pm}"
        got[pm] = alone
    assert torch.equal(got[False], got[True])


# ---- m2f_semantic_inference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_semantic_inference_against_the_float64_restatement(name):
    c = _case(name)
    r64, r32 = _restated(name, torch.float64), _restated(name, torch.float32)
    assert_gap(name, r64["full"], r32["full"])
    run = _first_run(name)
    assert tuple(run["sem_seg"].shape) == (B, min(c.C, 19)) + CROP and tuple(run["ood_score"].shape) == (B,) + CROP
    for k in ("sem_seg", "ood_score", "dcls_ood"):
        assert torch.isfinite(run[k]).all(), k
        held(f"{name} {k}", run[k], r64[k], r32[k])


@pytest.mark.parametrize("name", list(CASES))
def test_every_chunking_and_a_second_run_give_the_same_bits(name):
    run = _first_run(name)
    for per in (3, 2, 1):
        again = _run(name, per)
        for k in run:
            assert torch.equal(run[k], again[k]), (per, k)
    c = _case(name)
    d = lambda a: torch.from_numpy(a).to(DEV)
    alone = K.m2f_semantic_inference(d(c.cls), _pixel_major(d(c.x), c.ldq), IMAGE, CROP, Q=c.Q)       # without the ood head: sem_seg alone
    assert isinstance(alone, torch.Tensor) and torch.equal(alone.cpu(), run["sem_seg"])


@pytest.mark.parametrize("name", list(CASES))
def test_the_score_agrees_with_the_fused_forward_kernel(name):
    """kernels.m2f_score_fused: the same mathematics in another summation order (interpolate, sigmoid and mix per tile on the MFMA
    units). It takes a multiple of 4 queries: the 7-query case runs there with an eighth query of class probability exactly 0
    (its class logits -200 against 0 for "no object": expf underflows to 0) over a mask column of zeros."""
    c = _case(name)
    r64, r32 = _restated(name, torch.float64), _restated(name, torch.float32)
    assert_gap(name, r64["full"], r32["full"])
    cls_ood, x = torch.from_numpy(c.cls_ood).to(DEV), torch.from_numpy(c.x).to(DEV)
    if c.Q % 4:
        extra = torch.full((B, c.ldq - c.Q, c.C + 1), -200.0, device=DEV)
        extra[..., c.C] = 0
        cls_ood = torch.cat((cls_ood, extra), 1)
    fused = K.m2f_score_fused(cls_ood, _pixel_major(x, c.ldq, pad=0.0), IMAGE, CROP).cpu()
    held(f"{name} m2f_score_fused", fused, r64["ood_score"], r32["ood_score"])
    held(f"{name} ood_score", _first_run(name)["ood_score"], r64["ood_score"], r32["ood_score"])


def test_the_node_is_differentiable_in_the_ood_class_logits_only():
    c = _case("q7_c3_ldq8")
    d = lambda a: torch.from_numpy(a).to(DEV)
    cls, cls_ood = d(c.cls).requires_grad_(True), d(c.cls_ood).requires_grad_(True)
    lg = _pixel_major(d(c.x), c.ldq)
    sem, score = K.m2f_semantic_inference(cls, lg, IMAGE, CROP, class_logits_ood=cls_ood, Q=c.Q)
    assert sem.requires_grad is False and sem.grad_fn is None and score.requires_grad
    score.backward(d(c.g))
    assert cls.grad is None and cls_ood.grad is not None
    with pytest.raises(NotImplementedError):
        K.m2f_semantic_inference(cls, lg.clone().requires_grad_(True), IMAGE, CROP, class_logits_ood=cls_ood, Q=c.Q)
    with torch.no_grad():                                           # nothing to differentiate: the same values, no graph
        sem2, score2 = K.m2f_semantic_inference(cls, lg.clone().requires_grad_(True), IMAGE, CROP, class_logits_ood=cls_ood, Q=c.Q)
    assert torch.equal(sem2, sem) and torch.equal(score2, score) and not score2.requires_grad
    frozen = _run("q7_c3_ldq8", 3, grad=False)
    assert torch.equal(frozen["ood_score"], score.detach().cpu())
