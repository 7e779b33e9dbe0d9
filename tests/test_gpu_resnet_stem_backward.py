"""GPU: the backbone's backward with the stem weight trained (ResNet.set_trainable(stem=True)): stem.conv1.weight.grad against float64
autograd of the stock-torch restatement (tests/ref_resnet_grad.py) under the whole-backbone factor of tests/test_gpu_resnet_backward.py,
every other gradient and every map bit for bit what the stem-frozen path gives.

Conditions asserted first, on the CPU (conditions, not tolerances; no element is left out of a comparison): no ReLU input changes
sign between float32 and float64, the stem max-pool's arg-max is the same in both precisions in every window with a positive maximum,
and no window holds a positive tie."""
import pytest
import torch
import torch.nn.functional as F

import ref_resnet as R
import ref_resnet_grad as RG
from test_gpu_resnet_backward import BACKBONE_FACTOR, MODEL_SEED, NAMES, SIZES, _run, _same_pattern
from test_gpu_stem7_wgrad import positive_ties

pytestmark = pytest.mark.gpu

STEM_W = "stem.conv1.weight"


@pytest.fixture(scope="module")
def model():
    from multishiftseg_amd import build_resnet_backbone
    return R.randomize_(build_resnet_backbone(), MODEL_SEED).eval().cuda().set_trainable(stem=True)


def _pattern(model, kind):
    for p in model.parameters():
        p.requires_grad_(True)
    if kind == "faithful":
        return model.freeze(0, norms=True)
    model.freeze(1)                                            # "all": res2..res5 with their norms ...
    model.stem.conv1.weight.requires_grad_(kind == "all+stem")  # ... and the stem weight
    return model


@pytest.fixture(scope="module")
def refs(model):
    sd = {k: v.cpu() for k, v in model.state_dict().items()}
    out = {}
    for size in SIZES:
        g = torch.Generator().manual_seed(size[2] + MODEL_SEED)
        img = torch.randn(size, generator=g)
        with torch.no_grad():
            shapes = {n: t.shape for n, t in R.resnet50(img, R.cast(sd, torch.float32)).items()}
            a32 = F.relu(R.conv_norm(img, R.cast(sd, torch.float32), "stem.conv1", stride=2, padding=3))
            a64 = F.relu(R.conv_norm(img.double(), R.cast(sd, torch.float64), "stem.conv1", stride=2, padding=3))
        gm = {n: torch.randn(s, generator=g) for n, s in shapes.items()}
        o64, g64, t64 = RG.resnet50_grads(img, sd, gm, torch.float64)
        _, g32, t32 = RG.resnet50_grads(img, sd, gm, torch.float32)
        flips = RG.same_gates(t32, t64)
        m32, i32 = F.max_pool2d(a32, 3, 2, 1, return_indices=True)
        m64, i64 = F.max_pool2d(a64, 3, 2, 1, return_indices=True)
        differ = int((i32[m64 > 0] != i64[m64 > 0]).sum()) + int(((m32 > 0) != (m64 > 0)).sum())
        ties = int(positive_ties(a32).sum()) + int(positive_ties(a64).sum())
        print(f"{size}: {flips} ReLU sign flips, {differ} differing arg-maxes, {ties} positive ties")
        assert flips == 0, f"{size}: {flips} ReLU inputs change sign between float32 and float64 on the CPU: choose another seed"
        assert differ == 0 and ties == 0, f"{size}: {differ} stem pool windows with another arg-max in float32, {ties} positive ties"
        out[size] = (img, gm, o64, g64, g32)
    return out


@pytest.mark.parametrize("size", SIZES, ids=["70x100", "64x96"])
def test_stem_weight_gradient(model, refs, size, gemm_route):
    img, gm, o64, g64, g32 = refs[size]
    _pattern(model, "all+stem")
    maps, grads = _run(model, img, gm)
    for n in NAMES:
        _same_pattern(f"{size} {n}", maps[n], o64[n])
    got = grads[STEM_W]
    assert got is not None and got.shape == (64, 3, 7, 7) and got.dtype == torch.float32
    assert grads["stem.conv1.norm.weight"] is None and grads["stem.conv1.norm.bias"] is None
    e_hip, e_t32 = R.rel_max_err(got, g64[STEM_W]), R.rel_max_err(g32[STEM_W], g64[STEM_W])
    print(f"{gemm_route} {size} {STEM_W}: e_hip {e_hip:.3e}  e_t32 {e_t32:.3e}  ratio {e_hip / e_t32:.2f}")
    assert e_hip <= BACKBONE_FACTOR * e_t32
    # the other 156 gradients and the maps: the stem-frozen run, bit for bit
    _pattern(model, "all")
    maps0, grads0 = _run(model, img, gm)
    others = [n for n in grads if not n.startswith("stem.")]
    assert len(others) == 156 and grads0[STEM_W] is None
    for n in others:
        assert grads[n] is not None and torch.equal(grads[n], grads0[n]), n
    with torch.no_grad():
        frozen = model(img.cuda())
    for n in NAMES:
        assert torch.equal(maps[n], maps0[n]) and torch.equal(maps[n], frozen[n]), n


def test_the_faithful_pattern_trains_53_weights(model, refs):
    img, gm, _, _, _ = refs[SIZES[0]]
    _pattern(model, "all+stem")
    _, full = _run(model, img, gm)
    _pattern(model, "faithful")
    _, faithful = _run(model, img, gm)
    have = [n for n, g in faithful.items() if g is not None]
    assert len(have) == 53 and STEM_W in have and not any(".norm." in n for n in have)
    for n in have:
        assert torch.equal(faithful[n], full[n]), n


def test_a_trainable_stem_norm_raises(model, refs):
    img = refs[SIZES[1]][0].cuda()
    _pattern(model, "faithful")
    model.stem.conv1.norm.bias.requires_grad_(True)
    try:
        with pytest.raises(NotImplementedError, match="stem.conv1.norm.bias"):
            model(img)
    finally:
        model.stem.conv1.norm.bias.requires_grad_(False)
