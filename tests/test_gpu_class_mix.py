"""GPU: the class mix of SetCriterion.loss_ood (csrc/m2f_mix.hip, multishiftseg_amd/criterion.py) against the float64 restatement of
tests/ref_class_mix.py, wrapper by wrapper, as one autograd node and through the module.

Bounds: the rule of tests/test_gpu_criterion.py. The deviation max|hip - float64| of every output and every gradient tensor is at
most 8 x its own floor, floor = max|float32 restatement - float64| on the same inputs (asserted > 0); both are printed.
profiles/m2f_ood/tolerances.md keeps the record.

Conditions on the inputs (conditions, not tolerances). The gradient of -max_c is discontinuous where two classes tie, so the inputs
are built -- queries that belong to a class, masks that favour their class in bands of rows, noise on top -- and each case's seed
chosen, on a CPU with the restatement alone, such that in float64 the smallest gap between the two largest interpolated classes
over ALL output pixels is at least 64 x the float32 floor of those values; every test that differentiates -max_c asserts it. No
pixel is left out of any comparison. A loss value is a single float32 number, which even correctly rounded lies up to half an ulp
from the float64 one; as in tests/test_gpu_criterion.py the module case's seed is also chosen, on the restatement alone, such
that the floor of every loss_ood value is at least 0.3 ulp of the value, and that no score lies within 64 x floor of the kink
of the test's hinge loss (both asserted). One class-logit row holds a -80 entry (expf underflows), the mask logits hold +80, -80 and
an exact 0.0."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import poison
import ref_class_mix as ref
from multishiftseg_amd import HungarianMatcher, SetCriterion, class_mix_upsample
from multishiftseg_amd import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"

CASES = {
    # odd Q, a general C, a tile edge in both axes
    "q7_c3_tile_edges": dict(B=2, Q=7, C=3, hw=(11, 13), size=(44, 52), crop=(41, 50), seed=1),
    "q100_pixel_major": dict(B=2, Q=100, C=19, hw=(16, 24), size=(64, 96), crop=(64, 96), ldq=112, seed=1),
    # more than one tile and workgroup per image, more than one partial sum per (q, c)
    "q100_many_chunks": dict(B=4, Q=100, C=19, hw=(40, 72), size=(160, 288), crop=(157, 281), seed=3),
    "non_integer_scale": dict(B=2, Q=12, C=5, hw=(9, 10), size=(32, 37), crop=(32, 37), seed=1),
    # the logits keep 19 channels, the maximum runs over 21
    "c21": dict(B=2, Q=24, C=21, hw=(6, 7), size=(24, 28), crop=(23, 27), seed=2),
}


class Case:
    pass


def make_inputs(rng, B, Q, C, h, w):
    """(class logits [B,Q,C+1], mask logits [B,Q,h,w]) float32: query q belongs to class q % C; its mask favours the bands of rows
    that image b gives to that class."""
    cls = (rng.standard_normal((B, Q, C + 1)) * 0.6).astype(np.float32)
    owner = np.arange(Q) % C
    cls[:, np.arange(Q), owner] += 3
    cls[0, 0, (owner[0] + 1) % (C + 1)] = -80
    nb = min(C, 4)
    x = (rng.standard_normal((B, Q, h, w)) * 0.5).astype(np.float32)
    for b in range(B):
        band_class = rng.permutation(C)[:nb][(np.arange(h) * nb) // h]           # [h]
        x[b] += (2.0 * np.where(owner[:, None] == band_class[None, :], 1.0, -1.0)).astype(np.float32)[:, :, None]
    x[0, 0, 0, 0] = 80
    x[0, 1 % Q, h - 1, w - 1] = -80
    x[B - 1, Q - 1, h // 2, w // 2] = 0.0
    return cls, x


@functools.lru_cache(maxsize=None)
def _case(name):
    cfg = CASES[name]
    c = Case()
    c.name = name
    c.B, c.Q, c.C = cfg["B"], cfg["Q"], cfg["C"]
    (c.h, c.w), c.size, c.crop = cfg["hw"], cfg["size"], cfg["crop"]
    c.ldq = cfg.get("ldq")
    c.Cl = min(c.C, ref.LOGIT_CHANNELS)
    rng = np.random.default_rng(2000 + cfg["seed"])
    c.cls, c.x = make_inputs(rng, c.B, c.Q, c.C, c.h, c.w)
    c.dL = rng.standard_normal((c.B, c.Cl) + c.crop).astype(np.float32)
    c.ds = rng.standard_normal((c.B,) + c.crop).astype(np.float32)
    c.dM = rng.standard_normal((c.B, c.C, c.h, c.w)).astype(np.float32)
    m32, p32 = ref.mix(torch.from_numpy(c.cls), torch.from_numpy(c.x))
    c.mix32, c.prob32 = m32.numpy(), p32.numpy()                    # the inputs of the wrappers that are tested alone
    return c


@functools.lru_cache(maxsize=None)
def _restated(name, dtype):
    """Every output and gradient of the restatement at `dtype`, as float64 host tensors."""
    c = _case(name)
    t = lambda a: torch.from_numpy(a).to(dtype)
    cls, x = t(c.cls).requires_grad_(True), t(c.x).requires_grad_(True)
    M, P = ref.mix(cls, x)
    o = dict(mix=M, prob=P, full=ref.bilinear(M, c.size, c.crop))
    m_in = t(c.mix32).requires_grad_(True)
    o["up_logits"], o["up_neg_max"] = ref.upsample(m_in, c.size, c.crop, "logits"), ref.upsample(m_in, c.size, c.crop, "neg_max")
    o["full_alone"] = ref.bilinear(m_in, c.size, c.crop)
    o["dmix_logits"], = torch.autograd.grad(o["up_logits"], m_in, t(c.dL))
    o["dmix_neg_max"], = torch.autograd.grad(o["up_neg_max"], m_in, t(c.ds))
    o["dmix_both"] = o["dmix_logits"] + o["dmix_neg_max"]
    o["dx_alone"], o["dcls_alone"] = torch.autograd.grad(M, (x, cls), t(c.dM), retain_graph=True)
    for mode, cot in (("logits", c.dL), ("neg_max", c.ds)):
        out = ref.upsample(M, c.size, c.crop, mode)
        o[f"node_{mode}"] = out
        o[f"node_{mode}_dx"], o[f"node_{mode}_dcls"] = torch.autograd.grad(out, (x, cls), t(cot), retain_graph=True)
    return {k: v.detach().double() for k, v in o.items()}


def _pixel_major(m, ldq):
    """NCHW [B,Q,h,w] -> [B,h,w,ldq]; the padding of the query axis holds NaN: the kernels never read it."""
    B, Q, h, w = m.shape
    out = torch.full((B, h, w, ldq), float("nan"), device=m.device)
    out[..., :Q] = m.permute(0, 2, 3, 1)
    return out


def _from_layout(dx, Q, ldq):
    """A mask gradient in the layout of its input -> (NCHW, the pad columns or None)"""
    if ldq is None:
        return dx, None
    return dx[..., :Q].permute(0, 3, 1, 2).contiguous(), dx[..., Q:]


def _run_hip(name, ldq):
    """Every wrapper alone and the node in both modes -> dict of host tensors. ldq: the pixel-major layout with that pitch."""
    c = _case(name)
    d = lambda a: torch.from_numpy(a).to(DEV)
    cls, x = d(c.cls), d(c.x)
    pm = ldq is not None
    if pm:
        x = _pixel_major(x, ldq)
    o = {}
    o["mix"], o["prob"] = K.m2f_class_mix(cls, x, pixel_major=pm, Q=c.Q)
    mix32, dL, ds = d(c.mix32), d(c.dL), d(c.ds)
    o["up_logits"] = K.m2f_mix_upsample(mix32, c.size, c.crop, "logits")
    o["up_neg_max"] = K.m2f_mix_upsample(mix32, c.size, c.crop, "neg_max")
    o["dmix_logits"] = K.m2f_mix_upsample_backward(mix32, c.size, c.crop, dlogits=dL)
    o["dmix_neg_max"] = K.m2f_mix_upsample_backward(mix32, c.size, c.crop, dscore=ds)
    o["dmix_both"] = K.m2f_mix_upsample_backward(mix32, c.size, c.crop, dlogits=dL, dscore=ds)
    dx, o["dcls_alone"] = K.m2f_class_mix_backward(d(c.dM), d(c.prob32), cls, x, pixel_major=pm, Q=c.Q)
    o["dx_alone"], o["pad_alone"] = _from_layout(dx, c.Q, ldq)
    for mode, cot in (("logits", dL), ("neg_max", ds)):
        a, b = cls.clone().requires_grad_(True), x.clone().requires_grad_(True)
        out = class_mix_upsample(a, b, c.size, c.crop, mode, pixel_major=pm, Q=c.Q)
        out.backward(cot)
        o[f"node_{mode}"], o[f"node_{mode}_dcls"] = out.detach(), a.grad
        o[f"node_{mode}_dx"], o[f"pad_{mode}"] = _from_layout(b.grad, c.Q, ldq)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items() if v is not None}


@functools.lru_cache(maxsize=None)
def _first_run(name, ldq):
    return _run_hip(name, ldq)


COMPARED = ("mix", "prob", "up_logits", "up_neg_max", "dmix_logits", "dmix_neg_max", "dmix_both", "dx_alone", "dcls_alone", "node_logits",
            "node_logits_dx", "node_logits_dcls", "node_neg_max", "node_neg_max_dx", "node_neg_max_dcls")


def held(label, got, r64, r32):
    """The rule of the module docstring for one tensor."""
    assert got.shape == r64.shape, label
    dev, floor = float((got.double() - r64).abs().max()), float((r32 - r64).abs().max())
    print(f"{label}: max|hip - float64| {dev:.3e}, floor {floor:.3e}, bound {8 * floor:.3e}")
    assert floor > 0, label
    assert dev <= 8 * floor, label


def assert_gap(label, full64, full32):
    gap, floor = ref.top_gap(full64), float((full32 - full64).abs().max())
    print(f"{label}: smallest gap between the two largest classes {gap:.3e}, 64 x floor {64 * floor:.3e}")
    assert floor > 0 and gap >= 64 * floor, f"{label}: the -max_c check would go vacuous: choose another seed"


@pytest.mark.parametrize("name", list(CASES))
def test_wrappers_and_node_against_the_float64_restatement(name):
    c = _case(name)
    r64, r32 = _restated(name, torch.float64), _restated(name, torch.float32)
    assert_gap(f"{name} chain", r64["full"], r32["full"])
    assert_gap(f"{name} upsample alone", r64["full_alone"], r32["full_alone"])
    run = _first_run(name, c.ldq)
    for k in COMPARED:
        assert torch.isfinite(run[k]).all(), k
        held(f"{name} {k}", run[k], r64[k], r32[k])
    assert tuple(run["up_logits"].shape) == (c.B, c.Cl) + c.crop and tuple(run["up_neg_max"].shape) == (c.B,) + c.crop
    assert (run["dmix_logits"][:, c.Cl:] == 0).all()                # classes beyond the 19 logit maps get no gradient from them


@pytest.mark.parametrize("name", list(CASES))
def test_two_runs_and_both_layouts_give_the_same_bits(name):
    c = _case(name)
    run = _first_run(name, c.ldq)
    again = _run_hip(name, c.ldq)
    for k in run:
        assert torch.equal(run[k], again[k]), k
    other = _run_hip(name, None if c.ldq is not None else (c.Q + 3) // 4 * 4 + 4)
    for k in COMPARED:                                              # NCHW and pixel-major: L, s, dcls and the transposed dx
        assert torch.equal(run[k], other[k]), k
    for r in (run, other):
        for k in ("pad_alone", "pad_logits", "pad_neg_max"):
            if k in r:
                assert r[k].numel() > 0 and (r[k] == 0).all(), k    # exactly 0, not -0.0 times something, not NaN


def test_a_tie_gives_the_score_gradient_to_the_lower_class_index():
    rng = np.random.default_rng(5)
    B, C, h, w, size, crop = 2, 4, 7, 9, (28, 36), (27, 33)
    m = rng.random((B, C, h, w)).astype(np.float32)
    m[:, 1] += 2                                                    # classes 1 and 2 lead everywhere, bit-identical
    m[:, 2] = m[:, 1]
    ds = rng.standard_normal((B,) + crop).astype(np.float32)
    lowered = m.copy()
    lowered[:, 2] -= 1                                              # the same problem with the tie resolved by hand
    got = K.m2f_mix_upsample_backward(torch.from_numpy(m).to(DEV), size, crop, dscore=torch.from_numpy(ds).to(DEV)).cpu()
    want = K.m2f_mix_upsample_backward(torch.from_numpy(lowered).to(DEV), size, crop, dscore=torch.from_numpy(ds).to(DEV)).cpu()
    assert torch.equal(got, want)
    assert (got[:, 2] == 0).all() and (got[:, 0] == 0).all() and (got[:, 3] == 0).all() and (got[:, 1] != 0).any()
    res = {}
    for dtype in (torch.float64, torch.float32):
        mm = torch.from_numpy(m).to(dtype).requires_grad_(True)
        res[dtype], = torch.autograd.grad(ref.upsample(mm, size, crop, "neg_max"), mm, torch.from_numpy(ds).to(dtype))
    assert (res[torch.float64][:, 2] == 0).all()                    # the restatement applies the same rule
    held("tie dmix", got, res[torch.float64], res[torch.float32].double())
    # through the node: two class columns with bit-identical logits
    cls, x = make_inputs(rng, B, 6, C, h, w)
    cls[..., 1] += 4
    cls[..., 2] = cls[..., 1]
    a, b = torch.from_numpy(cls).to(DEV).requires_grad_(True), torch.from_numpy(x).to(DEV).requires_grad_(True)
    class_mix_upsample(a, b, size, crop, "neg_max").backward(torch.from_numpy(ds).to(DEV))
    grads = {}
    for dtype in (torch.float64, torch.float32):
        ra, rb = torch.from_numpy(cls).to(dtype).requires_grad_(True), torch.from_numpy(x).to(dtype).requires_grad_(True)
        grads[dtype] = torch.autograd.grad(ref.class_mix_upsample(ra, rb, size, crop, "neg_max"), (ra, rb), torch.from_numpy(ds).to(dtype))
    held("tie node dcls", a.grad.cpu(), grads[torch.float64][0], grads[torch.float32][0].double())
    held("tie node dx", b.grad.cpu(), grads[torch.float64][1], grads[torch.float32][1].double())


@pytest.mark.parametrize("name", ["q7_c3_tile_edges", "q100_pixel_major", "c21"])
def test_poisoned_scratch_and_padding_change_nothing(name):
    """Two clean runs and one run under each poison of tests/poison.py are bit-identical for every wrapper and for the node, in
    both layouts: no workspace, padding or output element is read before it is written, and no integer buffer is allocated
    uninitialised (poisoned() asserts that its list of unlisted sites stays empty)."""
    c = _case(name)
    d = lambda a: torch.from_numpy(a).to(DEV)
    cls, mix32, prob32, dL, ds, dM = d(c.cls), d(c.mix32), d(c.prob32), d(c.dL), d(c.ds), d(c.dM)
    first = _first_run(name, c.ldq)
    for ldq in (None, c.ldq or (c.Q + 3) // 4 * 4 + 4):
        pm = ldq is not None
        x = _pixel_major(d(c.x), ldq) if pm else d(c.x)
        runs = poison.poison_runs(lambda: list(K.m2f_class_mix(cls, x, pixel_major=pm, Q=c.Q)), bitwise=True)
        assert torch.equal(runs["clean"][0], first["mix"]) and torch.equal(runs["clean"][1], first["prob"])
        runs = poison.poison_runs(lambda: list(K.m2f_class_mix_backward(dM, prob32, cls, x, pixel_major=pm, Q=c.Q)), bitwise=True)
        assert torch.equal(runs["clean"][1], first["dcls_alone"])
        if pm:
            for tag in ("clean",) + poison.POISONS:
                assert (runs[tag][0][..., c.Q:] == 0).all()

        def node(mode, cot):
            a, b = cls.clone().requires_grad_(True), x.clone().requires_grad_(True)
            out = class_mix_upsample(a, b, c.size, c.crop, mode, pixel_major=pm, Q=c.Q)
            out.backward(cot)
            return [out.detach(), a.grad, b.grad]
        for mode, cot in (("logits", dL), ("neg_max", ds)):
            runs = poison.poison_runs(lambda: node(mode, cot), bitwise=True)
            assert torch.equal(runs["clean"][0], first[f"node_{mode}"]) and torch.equal(runs["clean"][1], first[f"node_{mode}_dcls"])
    for mode in ("logits", "neg_max"):
        runs = poison.poison_runs(lambda: K.m2f_mix_upsample(mix32, c.size, c.crop, mode), bitwise=True)
        assert torch.equal(runs["clean"][0], first[f"up_{mode}"])
    for k, kw in (("dmix_logits", dict(dlogits=dL)), ("dmix_neg_max", dict(dscore=ds)), ("dmix_both", dict(dlogits=dL, dscore=ds))):
        runs = poison.poison_runs(lambda: K.m2f_mix_upsample_backward(mix32, c.size, c.crop, **kw), bitwise=True)
        assert torch.equal(runs["clean"][0], first[k])


# ---- the module ------------------------------------------------------------------------------------------------------------------------
M_S, M_B, M_Q, M_C = 3, 2, 12, 5
M_HW, M_SIZE, M_CROP = (6, 7), (24, 28), (23, 26)
M_T, M_HW_T = [2, 1], (9, 4)
M_P, M_MATCH_P, M_OVER, M_KEEP = 65, 33, 3.0, 0.75
M_SEED = 12
HINGE = 2.0


def extra_loss(logits, score, target):
    """A small stock-torch stand-in for RelContrastiveLoss: a cross entropy on the logits plus a hinge on the score."""
    return F.cross_entropy(logits, target, ignore_index=255) + torch.relu(score + HINGE).mean()


@functools.lru_cache(maxsize=None)
def _module_case():
    rng = np.random.default_rng(3000 + M_SEED)
    c = Case()
    c.steps = []
    for _ in range(M_S):
        cls, x = make_inputs(rng, M_B, M_Q, M_C, *M_HW)
        cls_ood, x_ood = make_inputs(rng, M_B, M_Q, M_C, *M_HW)
        c.steps.append(dict(pred_logits=cls, pred_masks=x, pred_logits_ood=cls_ood, pred_masks_ood=x_ood))
    n = sum(M_T)
    c.tmasks = (rng.random((n,) + M_HW_T) < 0.5).astype(np.uint8)
    c.labels = rng.integers(0, M_C, n).astype(np.int64)
    c.sem = rng.integers(0, M_C, (M_B,) + M_CROP).astype(np.int64)
    c.sem[:, :3, :5] = 255
    K_, k_ = int(M_P * M_OVER), int(M_KEEP * M_P)
    c.cand = rng.random((M_S, n, K_, 2), dtype=np.float32)
    c.rnd = rng.random((M_S * n, M_P - k_, 2), dtype=np.float32)
    c.mpoints = rng.random((M_S, M_B, M_MATCH_P, 2), dtype=np.float32)
    return c


def _module_targets(c, device, sem_dtype=torch.int64):
    start = np.concatenate([[0], np.cumsum(M_T)])
    return [{"labels": torch.from_numpy(c.labels[start[b]:start[b + 1]]).to(device),
             "masks": torch.from_numpy(c.tmasks[start[b]:start[b + 1]]).to(device).bool(),
             "ood_mask": torch.zeros(M_SIZE, device=device), "sem_seg": torch.from_numpy(c.sem[b]).to(device).to(sem_dtype)} for b in range(M_B)]


def _module_criterion(losses, extra=extra_loss):
    crit = SetCriterion(M_C, HungarianMatcher(2.0, 5.0, 5.0, num_points=M_MATCH_P), {}, 0.1, losses, M_P, M_OVER, M_KEEP, "RCL", None, True).to(DEV)
    crit.set_extra_loss(extra)
    return crit


def _module_outputs(c, shared=False):
    steps = [{k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in st.items()} for st in c.steps]
    if shared:                                                      # this package's decoder: pred_masks_ood IS pred_masks
        for st in steps:
            st["pred_masks_ood"] = st["pred_masks"]
    return steps, dict(steps[0], aux_outputs=steps[1:])


def _inject(c):
    d = lambda a: torch.from_numpy(a).to(DEV)
    return dict(point_candidates=d(c.cand), random_points=d(c.rnd), matcher_points=d(c.mpoints))


OOD_KEYS = ["loss_ood"] + [f"loss_ood_{i}" for i in range(M_S - 1)]
COEF = {k: 1.0 + 0.37 * j for j, k in enumerate(OOD_KEYS)}
TENSORS = ("pred_logits", "pred_masks", "pred_logits_ood", "pred_masks_ood")


@functools.lru_cache(maxsize=None)
def _module_restated(dtype):
    c = _module_case()
    steps = [{k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in st.items()} for st in c.steps]
    sem = torch.from_numpy(c.sem)
    losses = {k: ref.loss_ood(st, M_SIZE, sem, extra_loss) for k, st in zip(OOD_KEYS, steps)}
    sum(COEF[k] * v for k, v in losses.items()).backward()
    fulls = [ref.bilinear(ref.mix(st["pred_logits_ood"], st["pred_masks_ood"])[0], M_SIZE, M_CROP).detach().double() for st in steps]
    return dict(losses={k: float(v.detach().double()) for k, v in losses.items()}, grads=[{k: st[k].grad.double() for k in TENSORS} for st in steps],
                fulls=fulls)


def test_module_with_deep_supervision_against_the_float64_restatement_and_no_host_synchronisation():
    c = _module_case()
    r64, r32 = _module_restated(torch.float64), _module_restated(torch.float32)
    for s in range(M_S):
        assert_gap(f"module step {s}", r64["fulls"][s], r32["fulls"][s])
        kink = float((HINGE - r64["fulls"][s].max(1).values).abs().min())       # the hinge of extra_loss is one more discontinuity
        floor = float((r32["fulls"][s] - r64["fulls"][s]).abs().max())
        print(f"module step {s}: smallest |score + {HINGE}| {kink:.3e}, 64 x floor {64 * floor:.3e}")
        assert kink >= 64 * floor, f"step {s}: a score lies on the kink of the hinge: choose another seed"
    crit = _module_criterion(["labels", "masks", "ood"])
    steps, outputs = _module_outputs(c)
    targets = _module_targets(c, DEV)
    inject = _inject(c)
    crit(outputs, targets, **inject)                                # a first call: lazy initialisation is not what is checked below
    torch.cuda.synchronize()
    checked = hasattr(torch.cuda, "set_sync_debug_mode")
    if checked:
        torch.cuda.set_sync_debug_mode("error")
    try:
        losses = crit(outputs, targets, **inject)
        sum(COEF[k] * losses[k] for k in OOD_KEYS).backward()
    finally:
        if checked:
            torch.cuda.set_sync_debug_mode("default")
    print(f"host synchronisation inside forward + backward: {'none (sync debug mode error)' if checked else 'UNCHECKED'}")
    plain = ["loss_ce", "loss_mask", "loss_dice"]
    assert list(losses) == plain + ["loss_ood"] + [f"{k}_{i}" for i in range(M_S - 1) for k in plain + ["loss_ood"]]
    assert all(v.dim() == 0 and v.is_cuda and v.requires_grad for v in losses.values())
    for k in OOD_KEYS:
        dev, floor = abs(float(losses[k].detach()) - r64["losses"][k]), abs(r32["losses"][k] - r64["losses"][k])
        ulp = float(np.spacing(np.float32(r64["losses"][k])))
        print(f"module {k}: |hip - float64| {dev:.3e}, floor {floor:.3e} ({floor / ulp:.2f} ulp), bound {8 * floor:.3e}")
        assert floor >= 0.3 * ulp, f"{k}: the float32 restatement happens to round almost exactly: choose another seed"
        assert dev <= 8 * floor, k
    for s in range(M_S):
        for k in TENSORS:
            held(f"module step {s} d/d {k}", steps[s][k].grad.cpu(), r64["grads"][s][k], r32["grads"][s][k])
    assert all(torch.equal(t["sem_seg"].cpu(), torch.from_numpy(c.sem[b])) for b, t in enumerate(targets))
    # the other losses: bit-identical to the same call without "ood", values and gradients
    steps2, outputs2 = _module_outputs(c)
    losses2 = _module_criterion(["labels", "masks"])(outputs2, targets, **inject)
    assert list(losses2) == [k for k in losses if "ood" not in k]
    assert all(torch.equal(losses2[k], losses[k]) for k in losses2)
    steps3, outputs3 = _module_outputs(c)
    losses3 = crit(outputs3, targets, **inject)
    sum(v for k, v in losses3.items() if "ood" not in k).backward()
    sum(losses2.values()).backward()
    for s in range(M_S):
        for k in ("pred_logits", "pred_masks"):
            assert torch.equal(steps2[s][k].grad, steps3[s][k].grad), (s, k)
    # pred_masks_ood is pred_masks: the same summed gradient as for a separate copy
    c2 = Case()
    c2.steps = [dict(st, pred_masks_ood=st["pred_masks"]) for st in c.steps]
    sep, out_sep = _module_outputs(c2)
    shr, out_shr = _module_outputs(c2, shared=True)
    for st, out in ((sep, out_sep), (shr, out_shr)):
        ls = crit(out, targets, **inject)
        sum(COEF[k] * ls[k] for k in OOD_KEYS).backward()
    for s in range(M_S):
        assert torch.equal(shr[s]["pred_masks"].grad, sep[s]["pred_masks"].grad + sep[s]["pred_masks_ood"].grad), s
        assert torch.equal(shr[s]["pred_logits"].grad, sep[s]["pred_logits"].grad) and torch.equal(shr[s]["pred_logits_ood"].grad, sep[s]["pred_logits_ood"].grad)
    # the pixel-major layout of a step: the same bits
    pm = [dict(pred_logits=st["pred_logits"].detach(), pred_logits_ood=st["pred_logits_ood"].detach(),
               pred_masks_pixel_major=_pixel_major(st["pred_masks"].detach(), M_Q + 4)) for st in shr]
    ls = crit(dict(pm[0], aux_outputs=pm[1:]), targets, **inject)
    ls_shr = crit(out_shr, targets, **inject)
    assert list(ls) == list(ls_shr) and all(torch.equal(ls[k], ls_shr[k]) for k in ls)


def test_module_with_the_real_rel_contrastive_loss():
    from multishiftseg_amd.loss import RelContrastiveLoss
    rng = np.random.default_rng(41)
    B, Q, C, hw, size, crop = 2, 24, 19, (12, 16), (48, 64), (45, 61)
    st = {}
    st["pred_logits"], st["pred_masks"] = make_inputs(rng, B, Q, C, *hw)
    st["pred_logits_ood"], st["pred_masks_ood"] = make_inputs(rng, B, Q, C, *hw)
    sem = rng.integers(0, C, (B,) + crop).astype(np.int64)
    sem[:, :4, :] = 255                                             # void rows in both images
    sem[1, 20:30, 10:40] = 254                                      # an OOD object in the augmented image
    params = {"ce_weights": [50, 10], "conduct_pixel_selection": False, "inoutaug_contras_margins_tri": [10, 5, 5]}
    rcl = RelContrastiveLoss(params, pairing="reference")
    crit = SetCriterion(C, HungarianMatcher(2.0, 5.0, 5.0, num_points=M_MATCH_P), {}, 0.1, ["ood"], M_P, M_OVER, M_KEEP, "RCL", None, False).to(DEV)
    crit.set_extra_loss(rcl)
    sem_dev = torch.from_numpy(sem).to(DEV)
    targets = [{"labels": torch.tensor([b], device=DEV), "masks": torch.ones((1,) + M_HW_T, device=DEV, dtype=torch.bool),
                "ood_mask": torch.zeros(size, device=DEV), "sem_seg": sem_dev[b]} for b in range(B)]
    outputs = {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in st.items()}
    torch.manual_seed(5)
    loss = crit(outputs, targets)["loss_ood"]
    loss.backward()
    assert loss.dim() == 0 and bool(torch.isfinite(loss))
    assert all(bool(torch.isfinite(outputs[k].grad).all()) and bool((outputs[k].grad != 0).any()) for k in TENSORS)
    assert torch.equal(sem_dev.cpu(), torch.from_numpy(sem))       # RelContrastiveLoss changed its own copy, not the caller's sem_seg
    plain = {k: torch.from_numpy(v).to(DEV) for k, v in st.items()}
    logits = ref.class_mix_upsample(plain["pred_logits"], plain["pred_masks"], size, crop, "logits").contiguous()
    score = ref.class_mix_upsample(plain["pred_logits_ood"], plain["pred_masks_ood"], size, crop, "neg_max").contiguous()
    torch.manual_seed(5)
    want = rcl(logits, score, torch.from_numpy(sem).to(DEV))
    print(f"loss_ood with RelContrastiveLoss: hip {float(loss):.9g}, stock-torch composition {float(want):.9g}")
    np.testing.assert_allclose(float(loss), float(want), rtol=1e-5)
    np_targets = [dict(t, sem_seg=sem[b]) for b, t in enumerate(targets)]          # numpy sem_seg, as the reference's data loader gives
    torch.manual_seed(5)
    np.testing.assert_allclose(float(crit(outputs, np_targets)["loss_ood"]), float(loss), rtol=1e-6)
