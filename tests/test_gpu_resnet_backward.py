"""GPU: the backward of the ResNet-50 backbone (multishiftseg_amd/resnet.py after set_trainable()) against float64 autograd of the
stock-torch restatement (tests/ref_resnet_grad.py) on the CPU.

Yardstick, as in tests/test_gpu_resnet.py and never our own output: per gradient tensor e = max|g - g64| / max|g64|; e_hip is ours,
e_t32 the same restatement under stock-torch float32 autograd. Asserted for one block alone: e_hip <= 4 * e_t32 -- both are fp32
accumulations of the same lengths; the factor covers a different summation order and one extra rounding per fold, as in the forward
test (measured: at most 2.33).

The whole backbone is asserted at 8 = 2 x 4 (DESIGN 3.23 has the figures and the cause). The forward test's factor 4 covers ONE pass
through the 16 blocks, and the forward maps already sit at 2.3-2.6 x e_t32 at res5; a gradient takes its operands and its gates from
that pass and then runs a second pass of the same length backwards through the same kernels, twice the roundings. Measured with
factor 4: native route 2 of 156 tensors over (worst 4.36, res5.0.conv1.norm.bias) at 70 x 100 and none (3.56) at 64 x 96; split-bf16
route 14 of 156 (worst 5.58) and 3 of 156 (worst 7.18, res3.1.conv1.norm.weight). e_hip is 0.7-2.9e-6 on every tensor, while e_t32
-- a maximum over one small tensor -- varies between 1.9e-7 and 9e-7 from tensor to tensor: every tensor over 4 has e_t32 <= 3.4e-7,
none has an e_hip outside the common range. No tensor has a bound of its own.

Gate-pattern condition (a condition, not a tolerance): a ReLU whose pre-activation changes sign between two precisions changes a
gradient by a finite amount. Every case first asserts, on the CPU, that the float32 restatement's `> 0` pattern at EVERY ReLU equals
the float64 one (the seeds below were chosen so that this holds) and, on the GPU, that the `> 0` pattern of the returned maps equals
the float64 one. A mismatch fails the test and says so; no element is ever left out of a comparison."""
import pytest
import torch

import ref_resnet as R
import ref_resnet_grad as RG

pytestmark = pytest.mark.gpu

FACTOR = 4                                         # one block alone
BACKBONE_FACTOR = 8                                # the whole backbone: two passes through the 16 blocks (docstring)
NAMES = ("res2", "res3", "res4", "res5")
SIZES = [(1, 3, 70, 100), (1, 3, 64, 96)]          # at the first every stride-2 layer sees an odd size
MODEL_SEED = 7                                     # with the images below: same ReLU patterns in float32 and float64 (checked on the CPU)
BLOCK_SEED = 1
KINDS = {"shortcut_stride2": (256, 64, 2), "shortcut_stride1": (256, 64, 1), "identity": (64, 16, 1)}


def _check_all(tag, got, g64, g32, factor=FACTOR):
    """Every tensor of g64: print the figures of all of them, then assert the bound on all of them. Returns the worst ratio."""
    rows = []
    for name in sorted(g64):
        assert got[name].shape == g64[name].shape and got[name].dtype == torch.float32, name
        e_hip, e_t32 = R.rel_max_err(got[name], g64[name]), R.rel_max_err(g32[name], g64[name])
        print(f"{tag} {name}: e_hip {e_hip:.3e}  e_t32 {e_t32:.3e}  ratio {e_hip / e_t32:.2f}")
        rows.append((e_hip / e_t32, name, e_hip, e_t32))
    over = [r for r in rows if r[2] > factor * r[3]]
    print(f"{tag}: worst ratio {max(rows)[0]:.2f} ({max(rows)[1]}), {len(over)} of {len(rows)} over {factor}")
    assert not over, (tag, over)
    return max(rows)[0]


def _same_pattern(tag, got, ref64):
    diff = int(((got.cpu() > 0) != (ref64 > 0)).sum())
    assert diff == 0, f"{tag}: {diff} outputs have another sign on the GPU than in float64 -- the gate patterns differ, choose another seed"


# ---- one block alone -----------------------------------------------------------------------------------------------------------
def _block_case(kind, hw):
    from multishiftseg_amd.resnet import BottleneckBlock
    cout, mid, stride = KINDS[kind]
    blk = R.randomize_(BottleneckBlock(64, cout, bottleneck_channels=mid, stride=stride), BLOCK_SEED, conv3_scale=1.0).eval()
    g = torch.Generator().manual_seed(100 + BLOCK_SEED)
    x = torch.randn((2, 64) + hw, generator=g)
    go = torch.randn((2, cout, (hw[0] - 1) // stride + 1, (hw[1] - 1) // stride + 1), generator=g)
    return blk, stride, x, go


def _block_reference(blk, stride, x, go):
    sd = {"b." + k: v for k, v in blk.state_dict().items()}
    o64, g64, t64 = RG.block_grads(x, sd, "b", stride, go, torch.float64)
    _, g32, t32 = RG.block_grads(x, sd, "b", stride, go, torch.float32)
    flips = RG.same_gates(t32, t64)
    assert flips == 0, f"{flips} ReLU inputs change sign between float32 and float64 on the CPU: choose another seed"
    return o64, g64, g32


def _block_backward(blk, x, go):
    from multishiftseg_amd import kernels as K
    tape, grads = [], {}
    with torch.no_grad():
        out = blk.forward_act_saving(K.nchw_to_act(x.cuda()), tape)
        dx = blk.backward_act(K.nchw_to_act(go.cuda()), *tape[0][1:], True, grads)
    named = {"b." + n: grads[p] for n, p in blk.named_parameters()}
    named["x"] = dx.nchw()
    return out.nchw(), named


@pytest.mark.parametrize("hw", [(9, 13), (8, 12)], ids=["9x13", "8x12"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_one_block_alone(kind, hw):
    """dx, the gradient of every weight and dgamma, dbeta of every norm of one block."""
    blk, stride, x, go = _block_case(kind, hw)
    o64, g64, g32 = _block_reference(blk, stride, x, go)
    out, got = _block_backward(blk.cuda(), x, go)
    _same_pattern(f"block {kind}", out, o64)
    assert set(got) == set(g64) and len(got) == (13 if kind != "identity" else 10)
    _check_all(f"block {kind} {hw}", got, g64, g32)


def test_weights_changed_in_place_are_packed_and_folded_again():
    """The stale-weight guards across steps: after an in-place update of one weight and one running_mean, as an optimizer step or a
    load makes them, a second forward + backward matches a fresh reference (and no longer the first)."""
    blk, stride, x, go = _block_case("shortcut_stride2", (9, 13))
    blk = blk.cuda()
    _, first = _block_backward(blk, x, go)
    with torch.no_grad():
        blk.conv2.weight.mul_(1.25)
        blk.shortcut.norm.running_mean.add_(0.05)
    o64, g64, g32 = _block_reference(blk, stride, x, go)
    out, got = _block_backward(blk, x, go)
    _same_pattern("block after the update", out, o64)
    _check_all("after the update", got, g64, g32)
    assert R.rel_max_err(first["x"], g64["x"]) > 100 * R.rel_max_err(g32["x"], g64["x"])      # the old packs are far outside the bound


# ---- the whole backbone --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from multishiftseg_amd import build_resnet_backbone
    return R.randomize_(build_resnet_backbone(), MODEL_SEED).eval().cuda().set_trainable()


def _pattern(model, kind):
    for p in model.parameters():
        p.requires_grad_(True)
    return {"all": lambda: model.freeze(1), "faithful": lambda: model.freeze(1, norms=True), "freeze2": lambda: model.freeze(2),
            "freeze3": lambda: model.freeze(3)}[kind]()


@pytest.fixture(scope="module")
def refs(model):
    """Per size: the image, the output gradients, and the float64 / float32 CPU gradients of every res2..res5 parameter."""
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    out = {}
    for size in SIZES:
        g = torch.Generator().manual_seed(size[2] + MODEL_SEED)
        img = torch.randn(size, generator=g)
        with torch.no_grad():
            shapes = {n: t.shape for n, t in R.resnet50(img, R.cast(sd, torch.float32)).items()}
        gm = {n: torch.randn(s, generator=g) for n, s in shapes.items()}
        o64, g64, t64 = RG.resnet50_grads(img, sd, gm, torch.float64)
        _, g32, t32 = RG.resnet50_grads(img, sd, gm, torch.float32)
        flips = RG.same_gates(t32, t64)
        assert flips == 0, f"{size}: {flips} ReLU inputs change sign between float32 and float64 on the CPU: choose another seed"
        out[size] = (img, gm, o64, g64, g32)
    return out


def _run(model, img, gm):
    """One forward + backward; ({name: map}, {parameter name: gradient or None})."""
    for p in model.parameters():
        p.grad = None
    maps = model(img.cuda())
    sum((maps[n] * g.cuda()).sum() for n, g in gm.items()).backward()
    return {n: t.detach() for n, t in maps.items()}, {n: p.grad for n, p in model.named_parameters()}


@pytest.mark.parametrize("size", SIZES, ids=["70x100", "64x96"])
def test_whole_backbone(model, refs, size, gemm_route):
    """Random gradients on all four maps, every res2..res5 parameter, on both GEMM routes under the same bound."""
    img, gm, o64, g64, g32 = refs[size]
    _pattern(model, "all")
    maps, grads = _run(model, img, gm)
    for n in NAMES:
        _same_pattern(f"{size} {n}", maps[n], o64[n])
    names = [n for n in grads if not n.startswith("stem.")]
    assert len(names) == 156 and all(grads[n] is not None for n in names)
    assert all(grads[n] is None for n in grads if n.startswith("stem."))
    assert sorted(names) == sorted(g for g in g64 if not g.startswith("stem."))
    _check_all(f"{gemm_route} {size}", grads, {n: g64[n] for n in names}, g32, BACKBONE_FACTOR)


def test_forward_maps_are_the_frozen_path_bit_for_bit(model, refs):
    img, gm, _, _, _ = refs[SIZES[0]]
    _pattern(model, "all")
    maps = model(img.cuda())
    assert all(maps[n].requires_grad for n in NAMES)
    with torch.no_grad():
        frozen = model(img.cuda())
    model.set_trainable(False)
    try:
        for p in model.parameters():
            p.requires_grad_(False)
        off = model(img.cuda())
    finally:
        model.set_trainable(True)
    for n in NAMES:
        assert torch.equal(maps[n], frozen[n]) and torch.equal(maps[n], off[n]) and not frozen[n].requires_grad


def test_freezing_patterns(model, refs):
    """The faithful stage-2 pattern builds no norm gradient. freeze() has detectron2's meaning (1: the stem, 2: and res2, 3: and res3):
    freeze(2) and freeze(3) leave res2 without gradients, and the stages they do not freeze match the fully-trainable run bit for bit."""
    img, gm, _, _, _ = refs[SIZES[0]]
    _pattern(model, "all")
    _, full = _run(model, img, gm)
    _pattern(model, "faithful")
    _, faithful = _run(model, img, gm)
    for n, g in faithful.items():
        if n.startswith("stem.") or ".norm." in n:
            assert g is None, n
        else:
            assert torch.equal(g, full[n]), n
    for kind, frozen in (("freeze2", ("stem.", "res2.")), ("freeze3", ("stem.", "res2.", "res3."))):
        _pattern(model, kind)
        _, part = _run(model, img, gm)
        for n, g in part.items():
            if n.startswith(frozen):
                assert g is None, (kind, n)
            else:
                assert torch.equal(g, full[n]), (kind, n)


def test_refusals(model, refs):
    img = refs[SIZES[1]][0].cuda()
    _pattern(model, "all")
    with pytest.raises(NotImplementedError, match="image"):
        model(img.clone().requires_grad_(True))
    model.stem.conv1.weight.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="stem"):
        model(img)
    model.stem.conv1.weight.requires_grad_(False)
    model.stem.conv1.norm.bias.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="stem"):
        model(img)
    _pattern(model, "all")
    model.train()
    try:
        with pytest.raises(NotImplementedError, match="train-mode"):
            model(img)
    finally:
        model.eval()
