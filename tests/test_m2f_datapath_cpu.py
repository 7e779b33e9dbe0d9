"""CPU: the host side of the Mask2Former input path (multishiftseg_amd/m2f_datapath.py) -- the draw order against the
restatement of tests/ref_augment.py, the refusals -- and self-checks of the oracle the GPU tests rely on."""
import random

import pytest
import torch

import ref_augment as R


def _same_draws(a, b):
    assert set(a) == set(b), (sorted(a), sorted(b))
    for k in ("p", "size", "top", "left", "entries"):
        assert a[k] == b[k], (k, a[k], b[k])
    if "geom" in a:
        assert tuple(a["geom"]) == tuple(b["geom"])
        assert (a["obj_mask"] == b["obj_mask"]).all() and (a["obj_img"] == b["obj_img"]).all()


def test_chain_is_the_trainers():
    from multishiftseg_amd import m2f_datapath as D
    assert tuple(D.M2F_CHAIN) == (("ToTensor", 1.0), ("ColorJitter", 0.5), ("GaussianBlur", 0.5), ("RandSharpness", 0.5), ("AutoContrast", 0.5),
                                  ("Equalize", 0.5), ("RandResize", 0.5), ("RandRotate", 0.5), ("RandHorizontalFlip", 0.5),
                                  ("RandVerticalFlip", 0.5), ("RandCrop", 1.0), ("Normalize", 1.0))
    assert tuple(D.M2F_CHAIN) == R.CHAIN and len(D.M2F_CHAIN) == 12


@pytest.mark.parametrize("objects", [False, True])
@pytest.mark.parametrize("force", [None, 0.0, 1.0])
def test_draw_order_matches_the_restatement(force, objects):
    """Same seeds -> same decisions and the same generator states afterwards (so the NEXT sample agrees too): over several
    seeds, with the chain's own probabilities and with every optional entry forced off / on, with and without the paste."""
    from multishiftseg_amd import m2f_datapath as D
    chain = D.M2F_CHAIN if force is None else tuple((n, p if p == 1.0 else force) for n, p in D.M2F_CHAIN)
    objs = R.rand_objects() if objects else None
    for seed in range(12):
        got, want = [], []
        for out, draw in ((got, lambda: D.draw_m2f_sample_params(40, 64, (24, 24), True, objs, R.scaled_object, rng=random, chain=chain)),
                          (want, lambda: R.draw_restated(40, 64, (24, 24), True, objs, R.scaled_object, random, chain=chain))):
            random.seed(seed)
            torch.manual_seed(seed)
            out += [draw() for _ in range(3)]       # three samples in a row from one stream
            out.append((random.random(), float(torch.rand(1))))
        for a, b in zip(got[:-1], want[:-1]):
            _same_draws(a, b)
        assert got[-1] == want[-1]
        if force == 1.0:
            assert [e["name"] for e in got[0]["entries"]] == [n for n, _ in chain]
        if force == 0.0:
            assert [e["name"] for e in got[0]["entries"]] == ["ToTensor", "RandCrop", "Normalize"]


def test_draws_without_mixup_and_with_an_own_rng():
    from multishiftseg_amd import m2f_datapath as D
    a = D.draw_m2f_sample_params(40, 64, (24, 24), mixup=False, rng=random.Random(5))
    torch.manual_seed(0)
    b = R.draw_restated(40, 64, (24, 24), False, None, None, random.Random(5))
    assert a["p"] is None and b["p"] is None
    assert [e["name"] for e in a["entries"]] == [e["name"] for e in b["entries"]]


def test_a_resized_sample_smaller_than_the_crop_is_refused():
    from multishiftseg_amd import m2f_datapath as D
    chain = tuple((n, 1.0) for n, _ in D.M2F_CHAIN)

    class Small(random.Random):
        def choice(self, seq):
            return seq[0]                       # scale 0.7: 40 x 64 -> 28 x 44
    with pytest.raises(ValueError, match="smaller than the crop"):
        D.draw_m2f_sample_params(40, 64, (30, 30), rng=Small(0), chain=chain)
    assert D.draw_m2f_sample_params(40, 64, (28, 44), rng=Small(0), chain=chain)["size"] == (28, 44)


def test_cpu_tensors_are_refused():
    from multishiftseg_amd import m2f_datapath as D
    img, gen, tgt, gtg = R.rand_maps(2, 40, 64)
    random.seed(0)
    torch.manual_seed(0)
    ps = [D.draw_m2f_sample_params(40, 64, (24, 24)) for _ in range(2)]
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):
        D.make_m2f_pair_batch(img, gen, tgt, gtg, (24, 24), ps)
    x, m = R.rand_stack(8, 8)
    for fn in (lambda: D.image_stats(x), lambda: D.autocontrast(x), lambda: D.gaussian_blur(x, 1.0), lambda: D.sharpness(x, 1.0),
               lambda: D.equalize(x), lambda: D.resize(x, m, (4, 4)), lambda: D.rotate(x, m, 3.0), lambda: D.window(x, m),
               lambda: D.load_pair(img[0], gen[0], tgt[0], gtg[0], 0.2)):
        with pytest.raises(RuntimeError, match="runs on an MI355X only"):
            fn()


# ---- oracle self-checks ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", R.SHAPES)
def test_oracle_f32_and_f64_agree(shape):
    """Every float op of the oracle in float32 against itself in float64: the e of the tolerance rule is a rounding figure
    (well below the 1e-3 a real defect shows), so max(8 e, 2^-20) is a tight bound."""
    x, m = R.rand_stack(*shape)
    es = {}
    for name, op, args in (("brightness", R.brightness, (1.8,)), ("contrast", R.contrast, (0.2,)), ("saturation", R.saturation, (1.8,)),
                           ("hue", R.hue, (-0.2,)), ("jitter", R.color_jitter, ([3, 1, 0, 2], (0.4, 1.7, 0.3, 0.13))),
                           ("autocontrast", R.autocontrast, ()), ("blur", R.gaussian_blur, (1.3,)), ("sharpness", R.sharpness, (2.0,)),
                           ("resize", R.resize, ((int(shape[0] * 0.7), int(shape[1] * 0.7)),)), ("rotate", R.rotate, (5.25,))):
        _, b, e = R.bound(op, x, *args)
        es[name] = e
        assert e < 1e-4 and b < 1e-3, (name, e)
    print(shape, {k: f"{v:.2e}" for k, v in es.items()})


def test_oracle_exact_identities():
    x, m = R.rand_bytes(23, 37)
    assert torch.equal(R.sharpness(x, 1.0), x) and torch.equal(R.resize(x, (23, 37)), x)
    assert torch.equal(R.sharpness(x[..., :2, :], 0.3), x[..., :2, :])
    assert torch.equal(R.equalize(x, dtype=torch.float64).float(), R.equalize(x))
    const = torch.full((1, 3, 9, 9), 0.5)
    assert torch.equal(R.equalize(const), (const * 255).to(torch.uint8).float() / 255)       # step == 0: the bytes stay
    assert torch.equal(R.autocontrast(const), const)                                           # scale not finite: unchanged
    y, mo = R.window(*R.window(x, m, hflip=True, vflip=True), hflip=True, vflip=True)
    assert torch.equal(y, x) and torch.equal(mo, m)


@pytest.mark.parametrize("shape", R.SHAPES)
def test_nearest_rotate_cap(shape):
    """The rule of the GPU test, checked on the CPU for the same inputs: leaving out the pixels whose float64 source
    coordinate lies within 1e-3 px of a rounding boundary drops at most 1 % of them, and on all others the float32 and the
    float64 oracle pick the same label."""
    x, m = R.rand_stack(*shape)
    for angle in R.ANGLES:
        keep = R.rotate_mask_decided(shape[0], shape[1], angle)
        assert 1.0 - float(keep.float().mean()) <= 0.01, (shape, angle)
        a, b = R.rotate_mask(m, angle, torch.float32), R.rotate_mask(m, angle, torch.float64)
        assert torch.equal(a[:, keep], b[:, keep]), (shape, angle)
    assert torch.equal(R.rotate_mask(m, 0.0), m)


def test_nearest_rotate_cap_on_the_chain_tests_draws():
    """The same check for the rotations the GPU chain tests draw (tests/test_gpu_m2f_datapath.py: B 2, 40 x 64, crop 24 x 24,
    seeds 0..4 with the chain's probabilities and seed 11 / 21 with every entry on)."""
    from multishiftseg_amd import m2f_datapath as D
    on = tuple((n, 1.0) for n, _ in D.M2F_CHAIN)
    seen = 0
    for seed, chain in [(s, D.M2F_CHAIN) for s in range(5)] + [(11, on), (21, on)]:
        random.seed(seed)
        torch.manual_seed(seed)
        for _ in range(2):
            prm = D.draw_m2f_sample_params(40, 64, (24, 24), True, R.rand_objects() if chain is on or seed % 2 == 0 else None, R.scaled_object, chain=chain)
            size = (40, 64)
            for e in prm["entries"]:
                size = e.get("size", size)
                if e["name"] == "RandRotate":
                    keep = R.rotate_mask_decided(size[0], size[1], e["angle"])
                    m = R.rand_stack(*size)[1]
                    assert 1.0 - float(keep.float().mean()) <= 0.01, (seed, size, e["angle"])
                    assert torch.equal(R.rotate_mask(m, e["angle"], torch.float32)[:, keep], R.rotate_mask(m, e["angle"], torch.float64)[:, keep])
                    seen += 1
    assert seen >= 4
