"""GPU: the resident object bank (multishiftseg_amd/object_bank.py, csrc/obj_bank.hip) against the numpy restatement
of its rules (tests/ref_object_bank.py): the bounding-box table, the rescaled and cut windows bit for bit with untouched
surroundings, the float64 bound, and both input pipelines end to end against host objects rescaled by the restatement."""
import random

import numpy as np
import pytest
import torch

import ref_object_bank as R

pytestmark = pytest.mark.gpu

SCALES = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0]
SIZES = [(10, 10), (13, 17), (37, 64), (64, 37), (100, 130)]
BIG = (480, 640)
# eight roundings (two products and a sum per pass, two passes, the two 1 - f), each at most 2^-24 relative, on values <= 255
F64_BOUND = 8 * 2.0 ** -24 * 255


def _mask(kind, H, W, rng):
    m = np.zeros((H, W), dtype=np.uint8)
    if kind == "valid":
        m[:] = 7
    elif kind == "corners":
        m[0, 0], m[0, W - 1], m[H - 1, 0], m[H - 1, W - 1] = 1, 7, 128, 254
    elif kind == "mix":
        m = rng.choice(np.array([0, 7, 254, 255], dtype=np.uint8), (H, W))
    return m                                              # "empty": zeros


def _single(y, x):
    m = np.zeros((12, 12), dtype=np.uint8)
    m[y, x] = 7
    return m


@pytest.fixture(scope="module")
def world():
    """objects (host), their names, the bank, and a cache of restated rescales."""
    from multishiftseg_amd.object_bank import ObjectBank
    rng = np.random.default_rng(2024)
    objs, names = [], []
    for H, W in SIZES:
        for kind in ("mix", "valid", "empty", "corners"):
            objs.append((rng.integers(0, 256, (H, W, 3), dtype=np.uint8), _mask(kind, H, W, rng)))
            names.append((H, W, kind))
    for y, x in ((4, 6), (5, 7)):
        objs.append((rng.integers(0, 256, (12, 12, 3), dtype=np.uint8), _single(y, x)))
        names.append((12, 12, f"single{y}{x}"))
    objs.append((rng.integers(0, 256, BIG + (3,), dtype=np.uint8), _mask("valid", *BIG, rng)))
    names.append(BIG + ("valid",))
    bank = ObjectBank(objs, SCALES, device="cuda")
    cache = {}

    def restated(index, scale):
        if (index, scale) not in cache:
            img, mask = objs[index]
            sh, sw = R.scaled_size(*mask.shape, scale)
            nm = R.nearest(mask, sh, sw)
            cache[(index, scale)] = (R.linear(img, sh, sw), R.linear_f64(img, sh, sw), nm, R.bbox(nm))
        return cache[(index, scale)]
    return dict(objs=objs, names=names, bank=bank, restated=restated, index={n: k for k, n in enumerate(names)})


def _checked_pairs(world):
    """every (object, scale) of the small sources; the 480 x 640 source at 0.1 and 1.0 only"""
    return [(k, s) for k, n in enumerate(world["names"]) for s in (SCALES if n[:2] != BIG else (0.1, 1.0))]


def test_bbox_table_equals_the_restatement(world):
    bank = world["bank"]
    assert len(bank) == len(world["objs"]) and bank.boxes.shape == (len(bank), len(SCALES), 4)
    assert bank.resident_bytes == 4 * sum(m.size for _, m in world["objs"]) == bank.img.numel() + bank.mask.numel()
    wrong = [(world["names"][k], s, bank.bbox(k, s), world["restated"](k, s)[3]) for k, s in _checked_pairs(world)
             if bank.bbox(k, s) != world["restated"](k, s)[3]]
    assert not wrong, wrong[:5]
    ix = world["index"]
    assert bank.bbox(ix[(12, 12, "single46")], 0.5) == (2, 3, 3, 4) and bank.bbox(ix[(12, 12, "single57")], 0.5) == (0, 0, 0, 0)
    # a scale outside the table: one launch, cached
    k = ix[(37, 64, "mix")]
    m = world["objs"][k][1]
    assert bank.bbox(k, 0.55) == R.bbox(R.nearest(m, *R.scaled_size(37, 64, 0.55))) and (k, 0.55) in bank._extra


def _check_windows(world, picks, img, mask, fill=None):
    """img / mask: what bank.rescale returned for picks. Windows equal the float32 restatement exactly, lie within F64_BOUND of the
    float64 form; with fill=(nan, byte) everything outside the windows still holds the fill."""
    img_h, mask_h = img.cpu(), mask.cpu()
    outside_i, outside_m = img_h.clone(), mask_h.clone()
    worst = 0.0
    for b, (k, s) in enumerate(picks):
        f32, f64, nm, (y1, x1, y2, x2) = world["restated"](k, s)
        bh, bw = y2 - y1, x2 - x1
        got = img_h[b, :bh, :bw]
        assert torch.equal(got, torch.from_numpy(f32[y1:y2, x1:x2])), (b, world["names"][k], s)
        assert torch.equal(mask_h[b, :bh, :bw], torch.from_numpy(nm[y1:y2, x1:x2])), (b, world["names"][k], s)
        if bh:
            worst = max(worst, float((got.double() - torch.from_numpy(f64[y1:y2, x1:x2])).abs().max()))
        outside_i[b, :bh, :bw] = float("nan")
        outside_m[b, :bh, :bw] = 0xA5
    print(f"max |kernel - float64 form| = {worst:.3e} (bound {F64_BOUND:.3e})")
    assert worst <= F64_BOUND
    if fill is not None:
        assert bool(torch.isnan(outside_i).all()) and bool((outside_m == 0xA5).all())


def test_rescale_writes_exactly_the_windows_into_filled_buffers(world):
    bank, ix = world["bank"], world["index"]
    picks = [(ix[BIG + ("valid",)], 1.0),                 # the largest window, scale 1.0
             (ix[(10, 10, "valid")], 0.1),                # a 1 x 1 window, the smallest
             (ix[(13, 17, "empty")], 0.5),                # an empty box
             (ix[BIG + ("valid",)], 0.1),
             (ix[(100, 130, "mix")], 1.0),
             (ix[(100, 130, "corners")], 0.7),
             (ix[(64, 37, "mix")], 0.3),
             (ix[(12, 12, "single46")], 0.5),             # a 1 x 1 window away from the origin of its object
             (ix[(12, 12, "single57")], 0.5)]             # empty after the rescale
    boxes = [bank.bbox(k, s) for k, s in picks]
    assert boxes[0] == (0, 0, 480, 640) and boxes[1] == (0, 0, 1, 1) and boxes[2] == (0, 0, 0, 0) and boxes[7] == (2, 3, 3, 4)
    B = len(picks)
    img = torch.full((B, 481, 643, 3), float("nan"), device="cuda")
    mask = torch.full((B, 481, 643), 0xA5, device="cuda", dtype=torch.uint8)
    got = bank.rescale(picks, out=(img, mask))
    assert got[0] is img and got[1] is mask
    _check_windows(world, picks, img, mask, fill=True)


def test_rescale_every_small_source_at_every_scale_in_one_launch(world):
    bank = world["bank"]
    picks = [(k, s) for k, s in _checked_pairs(world) if world["names"][k][:2] != BIG]
    img, mask = bank.rescale(picks)
    ohm = max(1, max(bank.bbox(k, s)[2] - bank.bbox(k, s)[0] for k, s in picks))
    owm = max(1, max(bank.bbox(k, s)[3] - bank.bbox(k, s)[1] for k, s in picks))
    assert tuple(img.shape) == (len(picks), ohm, owm, 3) and tuple(mask.shape) == (len(picks), ohm, owm)
    assert img.dtype == torch.float32 and mask.dtype == torch.uint8
    _check_windows(world, picks, img, mask)
    empty = [(world["index"][(13, 17, "empty")], 0.5)] * 2
    img, mask = bank.rescale(empty)                        # nothing to write: the buffers are 1 x 1 and stay as allocated
    assert tuple(img.shape) == (2, 1, 1, 3) and tuple(mask.shape) == (2, 1, 1)


def test_rescale_refuses_wrong_buffers(world):
    bank = world["bank"]
    picks = [(world["index"][(37, 64, "valid")], 1.0)]
    with pytest.raises(ValueError):
        bank.rescale(picks, out=(torch.zeros((1, 36, 64, 3), device="cuda"), torch.zeros((1, 36, 64), device="cuda", dtype=torch.uint8)))
    with pytest.raises(RuntimeError, match="no CPU path"):
        bank.rescale(picks, out=(torch.zeros((1, 37, 64, 3)), torch.zeros((1, 37, 64), dtype=torch.uint8)))
    with pytest.raises(TypeError):
        bank.rescale(picks, out=(torch.zeros((1, 37, 64, 3), device="cuda", dtype=torch.float64),
                                 torch.zeros((1, 37, 64), device="cuda", dtype=torch.uint8)))


# ---- end to end ------------------------------------------------------------------------------------------------------------------

H, W, CROP = 96, 128, (64, 64)


@pytest.fixture(scope="module")
def paste_world(world):
    """Objects that fit the 64 x 64 crop, as host objects and as a bank; seeded uint8 maps for a batch of four."""
    from multishiftseg_amd.object_bank import ObjectBank
    keep = [k for k, n in enumerate(world["names"]) if n[0] <= 64 and n[1] <= 64]
    objs = [world["objs"][k] for k in keep]
    g = torch.Generator().manual_seed(7)
    maps = (torch.randint(0, 256, (4, H, W, 3), generator=g, dtype=torch.uint8), torch.randint(0, 256, (4, H, W, 3), generator=g, dtype=torch.uint8),
            torch.randint(0, 19, (4, H, W), generator=g, dtype=torch.uint8), torch.randint(0, 19, (4, H, W), generator=g, dtype=torch.uint8))
    return dict(objs=objs, bank=ObjectBank(objs, device="cuda"), maps=tuple(t.cuda() for t in maps))


def _both(draw, B, seed):
    """(parameter sets with host objects, parameter sets with picks) under the same seed"""
    out = []
    for kind in ("host", "bank"):
        rng = random.Random(seed)
        torch.manual_seed(seed)
        out.append([draw(kind, rng) for _ in range(B)])
    return out


def test_deeplab_pipeline_with_the_bank_equals_host_objects(paste_world):
    from multishiftseg_amd import datapath as D
    pw = paste_world

    def draw(kind, rng):
        if kind == "host":
            return D.draw_sample_params(H, W, CROP, True, pw["objs"], R.scaled_object, rng=rng)
        return D.draw_sample_params(H, W, CROP, True, pw["bank"], rng=rng)

    def wanted(seed):                                      # one sample with an empty box, the others with a window
        sizes = [p["geom"][2] for p in _both(draw, 4, seed)[1]]
        return sizes.count(0) == 1
    seed = next(s for s in range(500) if wanted(s))
    host, bank = _both(draw, 4, seed)
    assert [p["geom"][2:] for p in host] == [p["geom"][2:] for p in bank] and all("pick" in p and "obj_img" not in p for p in bank)
    want_img, want_tgt = D.make_pair_batch(*pw["maps"], CROP, host)
    got_img, got_tgt = D.make_pair_batch(*pw["maps"], CROP, bank, bank=pw["bank"])
    assert torch.equal(got_img, want_img) and torch.equal(got_tgt, want_tgt)
    plain = D.make_pair_batch(*pw["maps"], CROP, [{k: v for k, v in p.items() if k in ("p", "top", "left")} for p in host])
    assert not torch.equal(plain[0], want_img) and not torch.equal(plain[1], want_tgt)        # the paste is visible at all
    with pytest.raises(ValueError, match="bank"):
        D.make_pair_batch(*pw["maps"], CROP, bank)
    with pytest.raises(ValueError, match="either"):
        D.make_pair_batch(*pw["maps"], CROP, bank[:2] + host[2:], bank=pw["bank"])


@pytest.mark.parametrize("chain", ["three", "default"])
def test_m2f_pipeline_with_the_bank_equals_host_objects(paste_world, chain):
    from multishiftseg_amd import m2f_datapath as M
    pw = paste_world
    ch = M.M2F_CHAIN if chain == "default" else (("ToTensor", 1.0), ("RandCrop", 1.0), ("Normalize", 1.0))

    def draw(kind, rng):
        if kind == "host":
            return M.draw_m2f_sample_params(H, W, CROP, True, pw["objs"], R.scaled_object, rng=rng, chain=ch)
        return M.draw_m2f_sample_params(H, W, CROP, True, pw["bank"], rng=rng, chain=ch)
    seed = next(s for s in range(500) if all(p["geom"][2] > 0 for p in _both(draw, 2, s)[1]))
    host, bank = _both(draw, 2, seed)
    assert [p["entries"] for p in host] == [p["entries"] for p in bank]
    maps = tuple(t[:2].contiguous() for t in pw["maps"])
    want_img, want_tgt = M.make_m2f_pair_batch(*maps, CROP, host)
    got_img, got_tgt = M.make_m2f_pair_batch(*maps, CROP, bank, bank=pw["bank"])
    assert torch.equal(got_img, want_img) and torch.equal(got_tgt, want_tgt)
    with pytest.raises(ValueError, match="bank"):
        M.make_m2f_pair_batch(*maps, CROP, bank)
