"""GPU: every kernel family of libmss_aug.so alone, and the Mask2Former input chain stage by stage, against the stock-torch
oracle tests/ref_augment.py.

Float stages: max |device - oracle_f64| <= max(8 e, 2^-20) with e = max |oracle_f32 - oracle_f64| on the same input
(ref_augment.bound); exact stages: torch.equal. Nearest rotate: equality on every pixel whose float64 source coordinate is at
least 1e-3 px away from a rounding boundary (at most 1 % may be left out; tests/test_m2f_datapath_cpu.py repeats that on the
CPU). Shapes: 23x37 (odd, below one tile), 37x53, 64x96 (H W a multiple of 4: the 16-byte path) and 70x151 (two workgroups in
each grid dimension, H W not a multiple of 4)."""
import itertools
import random

import pytest
import torch

import ref_augment as R

pytestmark = pytest.mark.gpu

SHAPES = R.SHAPES


@pytest.fixture(scope="module")
def D():
    from multishiftseg_amd import m2f_datapath
    return m2f_datapath


@pytest.fixture(scope="module")
def stacks():
    """The shared CPU inputs, made once and never modified (every device op gets its own copy)."""
    return {s: R.rand_stack(*s) for s in SHAPES}


def close(got, op, x, *args, what=""):
    want, b, e = R.bound(op, x, *args)
    err = float((got.detach().cpu().double() - want).abs().max())
    print(f"{what or op.__name__} {tuple(x.shape[-2:])} {args}: err {err:.3e}  e {e:.3e}  bound {b:.3e}")
    assert torch.isfinite(got).all()
    assert err <= b, (what or op.__name__, tuple(x.shape), args, err, b)


def test_load_is_exact(D):
    for (H, W), p in itertools.product(((23, 37), (70, 151)), (None, 0.3, 0.13436424411240122, 0.0, 1.0)):
        img, gen, tgt, gtg = (t[0] for t in R.rand_maps(1, H, W, seed=H))
        x, m = D.load_pair(img.cuda(), gen.cuda(), tgt.cuda(), gtg.cuda(), p)
        rx, rm = R.load(img, gen, tgt, gtg, p)
        assert torch.equal(x.cpu(), rx) and torch.equal(m.cpu(), rm), (H, W, p)


@pytest.mark.parametrize("shape", SHAPES + ((300, 300),))
def test_stats(D, stacks, shape):
    x = stacks[shape][0] if shape in stacks else R.rand_stack(*shape)[0]
    x = x * 0.7 + 0.1
    s = D.image_stats(x.cuda())
    s2 = D.image_stats(x.cuda())
    assert torch.equal(s, s2)                                            # fixed-order reduction: the same bits
    s = s.cpu()
    for c in range(3):
        assert torch.equal(s[:, 1 + 2 * c], x[:, c].amin(dim=(-2, -1))) and torch.equal(s[:, 2 + 2 * c], x[:, c].amax(dim=(-2, -1)))
    mean = lambda x, dtype: R.gray(x.to(dtype)).mean(dim=(-3, -2, -1))
    close(s[:, 0], mean, x, what="gray mean")


@pytest.mark.parametrize("shape", SHAPES)
def test_colour_ops_alone(D, stacks, shape):
    x = stacks[shape][0]
    A = D.A
    for kind, op, factors in ((A.OP_BRIGHTNESS, R.brightness, (0.2, 1.8, 1.0, 0.0)), (A.OP_CONTRAST, R.contrast, (0.2, 1.8, 1.0, 0.0)),
                              (A.OP_SATURATION, R.saturation, (0.2, 1.8, 1.0, 0.0)), (A.OP_HUE, R.hue, (-0.2, 0.2, 0.0, 0.5, -0.5))):
        for f in factors:
            close(D.pointwise(x.cuda(), [(kind, f)]), op, x, f)
    close(D.autocontrast(x.cuda()), R.autocontrast, x)
    y = (x * 0.6 + 0.2).contiguous()
    close(D.autocontrast(y.cuda()), R.autocontrast, y, what="autocontrast, narrow range")


def test_colour_degenerate_inputs(D):
    const = torch.full((2, 3, 23, 37), 0.37)
    for f in (0.2, 1.8):
        close(D.pointwise(const.cuda(), [(D.A.OP_CONTRAST, f)]), R.contrast, const, f, what="contrast of a constant image")
    x = R.rand_stack(23, 37)[0] * 0.5 + 0.25
    x[:, 1] = 0.6                                                         # a constant channel: scale not finite -> unchanged
    got = D.autocontrast(x.cuda())
    close(got, R.autocontrast, x, what="autocontrast with a constant channel")
    assert torch.equal(got[:, 1].cpu(), x[:, 1])
    g = torch.rand(2, 1, 23, 37).expand(2, 3, 23, 37).contiguous()      # all gray: hue and saturation leave it alone
    close(D.pointwise(g.cuda(), [(D.A.OP_HUE, 0.17)]), R.hue, g, 0.17, what="hue of a gray image")


def test_color_jitter_all_permutations(D, stacks):
    x = stacks[(23, 37)][0]
    f = (0.4, 1.7, 0.3, 0.13)
    for perm in itertools.permutations(range(4)):
        close(D.color_jitter(x.cuda(), list(perm), *f), R.color_jitter, x, list(perm), f)
    x = stacks[(64, 96)][0]                                              # the 16-byte path, range ends
    close(D.color_jitter(x.cuda(), [3, 2, 1, 0], 1.8, 0.2, 1.8, -0.2), R.color_jitter, x, [3, 2, 1, 0], (1.8, 0.2, 1.8, -0.2))


def test_pointwise_run_of_more_than_eight_ops(D, stacks):
    x = stacks[(37, 53)][0]
    A = D.A
    ops = [(A.OP_BRIGHTNESS, 0.9), (A.OP_SATURATION, 1.1), (A.OP_HUE, 0.05)] * 3 + [(A.OP_BRIGHTNESS, 1.1)]

    def ref(x, dtype):
        for kind, f in ops:
            x = {A.OP_BRIGHTNESS: R.brightness, A.OP_SATURATION: R.saturation, A.OP_HUE: R.hue}[kind](x, f, dtype=dtype)
        return x
    close(D.pointwise(x.cuda(), ops), ref, x, what="ten ops, two passes")


@pytest.mark.parametrize("shape", SHAPES + ((5, 5), (9, 12)))
def test_blur(D, stacks, shape):
    x = stacks[shape][0] if shape in stacks else R.rand_stack(*shape)[0]
    for sigma in (0.1, 1.3, 5.0):
        close(D.gaussian_blur(x.cuda(), sigma), R.gaussian_blur, x, sigma)


def test_blur_reflects_at_every_border(D):
    """Unit impulses at the four corners and the four edge midpoints: every reflect index of the padding is exercised."""
    for H, W in ((9, 12), (5, 5), (23, 70)):
        spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)]
        x = torch.zeros(len(spots), 3, H, W)
        for n, (i, j) in enumerate(spots):
            x[n, :, i, j] = 1.0
        close(D.gaussian_blur(x.cuda(), 5.0), R.gaussian_blur, x, 5.0, what="impulses")


def test_blur_refuses_images_below_five_pixels(D):
    from multishiftseg_amd._lib_aug import MssError
    for shape in ((4, 9), (9, 4)):
        with pytest.raises(MssError, match="unsupported shape"):
            D.gaussian_blur(torch.zeros(2, 3, *shape).cuda(), 1.0)


@pytest.mark.parametrize("shape", SHAPES + ((3, 3),))
def test_sharpness(D, stacks, shape):
    x = stacks[shape][0] if shape in stacks else R.rand_stack(*shape)[0]
    for f in (0.0, 1.0, 2.0, 0.8989821295774763):
        got = D.sharpness(x.cuda(), f)
        close(got, R.sharpness, x, f)
        if f == 1.0:
            assert torch.equal(got.cpu(), x)


def test_sharpness_leaves_thin_images_alone(D):
    for shape in ((2, 9), (9, 2), (1, 1)):
        x = R.rand_stack(*shape)[0]
        assert torch.equal(D.sharpness(x.cuda(), 1.7).cpu(), x), shape


def _eq_check(D, x):
    assert torch.equal(D.equalize(x.cuda()).cpu(), R.equalize(x))


@pytest.mark.parametrize("shape", SHAPES)
def test_equalize_random_bytes(D, shape):
    _eq_check(D, R.rand_bytes(*shape)[0])


def test_equalize_special_histograms(D):
    g = torch.Generator().manual_seed(3)
    x = R.rand_bytes(37, 53)[0]
    x[:, 1] = 77 / 255.0                                                  # a constant channel: step == 0
    _eq_check(D, x)
    two = torch.where(torch.rand(2, 3, 37, 53, generator=g) < 0.3, torch.tensor(10 / 255.0), torch.tensor(200 / 255.0))
    _eq_check(D, two.contiguous())
    levels = (torch.arange(2 * 3 * 64 * 96).reshape(2, 3, 64, 96) % 256).to(torch.float32) / 255      # all 256 levels, equally often
    _eq_check(D, levels)
    few = torch.zeros(1, 3, 16, 16)
    few.view(1, 3, -1)[:, :, :256] = torch.arange(256).float() / 255      # one pixel per level: step 1
    _eq_check(D, few)


def test_equalize_counts_beyond_16_bits(D):
    x = R.rand_bytes(300, 300, seed=5)[0]
    x[:, 0] = torch.where(x[:, 0] < 0.8, torch.tensor(51 / 255.0), x[:, 0])      # one bin above 2^16
    assert int(((x[0, 0] * 255).round() == 51).sum()) > 65536
    _eq_check(D, x.contiguous())


@pytest.mark.parametrize("shape", SHAPES)
def test_resize(D, stacks, shape):
    x, m = stacks[shape]
    for scale in (0.7, 0.8, 0.9, 1.0):
        size = (int(shape[0] * scale), int(shape[1] * scale))
        y, mo = D.resize(x.cuda(), m.cuda(), size)
        close(y, R.resize, x, size)
        assert torch.equal(mo.cpu(), R.resize_mask(m, size)), (shape, scale)
        if scale == 1.0:
            assert torch.equal(y.cpu(), x)


@pytest.mark.parametrize("shape", SHAPES)
def test_rotate(D, stacks, shape):
    x, m = stacks[shape]
    for angle in R.ANGLES:
        y, mo = D.rotate(x.cuda(), m.cuda(), angle)
        close(y, R.rotate, x, angle)
        keep = R.rotate_mask_decided(shape[0], shape[1], angle)
        assert 1.0 - float(keep.float().mean()) <= 0.01
        want = R.rotate_mask(m, angle, torch.float64)
        assert torch.equal(mo.cpu()[:, keep], want[:, keep]), (shape, angle)
    y, mo = D.rotate(x.cuda(), m.cuda(), 0.0)
    assert torch.equal(mo.cpu(), m)


def test_rotated_in_corners_are_black_and_class_0(D):
    x = torch.full((2, 3, 37, 53), 0.5)
    m = torch.full((2, 37, 53), 7, dtype=torch.uint8)
    y, mo = D.rotate(x.cuda(), m.cuda(), 10.0)
    assert int(mo[0, 0, 0]) == 0 and float(y[0, 0, 0, 0]) == 0.0 and int(mo[0, 18, 26]) == 7


def _finish_ref(x, m, B, b, hflip, vflip, top, left, size, paste):
    wx, wm = R.window(x, m, hflip, vflip, top, left, size)
    img, tgt = R.normalize(wx), wm.to(torch.int64)
    if paste is not None:
        i0, t0 = R.paste(img[0], tgt[0], *paste)
        img, tgt = torch.stack([i0, img[1]]), torch.stack([t0, tgt[1]])
    return img, tgt


@pytest.mark.parametrize("shape", ((23, 37), (70, 300)))
def test_window_and_finish_are_exact(D, shape):
    x, m = R.rand_stack(*shape)
    m = m % 200                                     # below the object's class id 254
    H, W = shape
    h, w = H - 6, W - 9
    obj_img, obj_mask = R.rand_objects(1)[0]
    oh, ow = obj_mask.shape
    y1, x1, y2, x2 = 2, 1, oh - 1, ow - 2
    bh, bw = y2 - y1, x2 - x1
    xd, md = x.cuda(), m.cuda()
    for hflip, vflip in itertools.product((False, True), repeat=2):
        for top, left, size in ((0, 0, (h, w)), (H - h, W - w, (h, w)), (0, 0, (H, W)), (3, 4, (h, w))):
            y, mo = D.window(xd, md, hflip, vflip, top, left, size)
            ry, rm = R.window(x, m, hflip, vflip, top, left, size)
            assert torch.equal(y.cpu(), ry) and torch.equal(mo.cpu(), rm)
            ch, cw = size
            corners = [None, (0, 0), (0, cw - bw), (ch - bh, 0), (ch - bh, cw - bw), (ch // 3, cw // 3)]     # touching each border
            for corner in corners if (hflip, vflip) in ((False, False), (True, True)) else corners[:2]:
                paste = None if corner is None else (obj_img, obj_mask, (y1, x1, bh, bw) + corner)
                out_img = torch.full((6, 3, ch, cw), float("nan")).cuda()
                out_tgt = torch.full((6, ch, cw), -1, dtype=torch.int64).cuda()
                kw = {} if paste is None else dict(obj_img=torch.from_numpy(obj_img).cuda(), obj_mask=torch.from_numpy(obj_mask).cuda(), geom=paste[2])
                D.finish(xd, md, out_img, out_tgt, 1, hflip, vflip, top, left, size, **kw)
                ri, rt = _finish_ref(x, m, 3, 1, hflip, vflip, top, left, size, paste)
                assert torch.equal(out_img[[1, 4]].cpu(), ri) and torch.equal(out_tgt[[1, 4]].cpu(), rt), (hflip, vflip, top, left, size, corner)
                assert torch.isnan(out_img[[0, 2, 3, 5]]).all() and (out_tgt[[0, 2, 3, 5]] == -1).all()     # only the sample's two slots
                if paste is not None:
                    assert (rt[0] == 254).any() and not (rt[1] == 254).any()


# ---- the chain ---------------------------------------------------------------------------------------------------------------------

B, H, W, CROP = 2, 40, 64, (24, 24)


def _draw(D, seed, chain=None, objects=True):
    random.seed(seed)
    torch.manual_seed(seed)
    objs = R.rand_objects() if objects else None
    return [D.draw_m2f_sample_params(H, W, CROP, True, objs, R.scaled_object, chain=chain or D.M2F_CHAIN) for _ in range(B)]


def _run(D, maps, params, trace=None):
    return D.make_m2f_pair_batch(*(t.cuda() for t in maps), CROP, params, trace=trace)


def _check_stagewise(D, maps, params):
    trace = []
    out_img, out_tgt = _run(D, maps, params, trace)
    assert torch.isfinite(out_img).all()
    fused_img, fused_tgt = _run(D, maps, params)
    assert torch.equal(fused_img, out_img) and torch.equal(fused_tgt, out_tgt)        # stage by stage == fused, bit for bit
    it = iter(trace)
    for b, prm in enumerate(params):
        name, x, m = next(it)
        px, pm = x.cpu(), m.cpu()
        rx, rm = R.load(maps[0][b], maps[1][b], maps[2][b], maps[3][b], prm["p"])
        assert name == "ToTensor" and torch.equal(px, rx) and torch.equal(pm, rm)
        for e in prm["entries"][1:]:
            name, x, m = next(it)
            assert name == e["name"]
            x, m = x.cpu(), m.cpu()
            if name in R.EXACT:
                rx, rm = R.apply_entry(px, pm, e, CROP)
                assert torch.equal(x, rx) and torch.equal(m, rm), (b, name)
            else:
                close(x, lambda t, dtype: R.apply_entry(t, pm, e, CROP, dtype=dtype)[0], px, what=f"chain {name}")
                rm = R.apply_entry(px, pm, e, CROP, dtype=torch.float64)[1]
                if name == "RandRotate":
                    keep = R.rotate_mask_decided(pm.shape[1], pm.shape[2], e["angle"])
                    assert 1.0 - float(keep.float().mean()) <= 0.01
                    assert torch.equal(m[:, keep], rm[:, keep])
                else:
                    assert torch.equal(m, rm), (b, name)
            px, pm = x, m
        img, tgt = px, pm.to(torch.int64)                     # the device's Normalize stage (checked exactly above), then the paste
        if "geom" in prm:
            i0, t0 = R.paste(img[0], tgt[0], prm["obj_img"], prm["obj_mask"], prm["geom"])
            img, tgt = torch.stack([i0, img[1]]), torch.stack([t0, tgt[1]])
        assert torch.equal(out_img[[b, B + b]].cpu(), img) and torch.equal(out_tgt[[b, B + b]].cpu(), tgt), b
    assert next(it, None) is None
    assert out_tgt.dtype == torch.int64 and int(out_tgt.min()) >= 0 and int(out_tgt.max()) <= 255


def test_chain_stagewise_every_entry_on(D):
    chain = tuple((n, 1.0) for n, _ in D.M2F_CHAIN)
    maps = R.rand_maps(B, H, W)
    params = _draw(D, 11, chain)                                 # 0.7 x 40 = 28 >= 24: every scale fits this crop
    assert all(len(p["entries"]) == 12 for p in params)
    _check_stagewise(D, maps, params)


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_chain_stagewise_drawn_decisions(D, seed):
    _check_stagewise(D, R.rand_maps(B, H, W, seed), _draw(D, seed, objects=seed % 2 == 0))


def test_chain_is_deterministic_and_survives_poison(D):
    import poison
    maps = tuple(t.cuda() for t in R.rand_maps(B, H, W, 9))
    params = _draw(D, 21, tuple((n, 1.0) for n, _ in D.M2F_CHAIN))
    runs = poison.poison_runs(lambda: D.make_m2f_pair_batch(*maps, CROP, params), bitwise=True)
    assert all(runs["reproducible"]) and torch.isfinite(runs["clean"][0]).all()


def test_batch_feeds_prepare_targets(D):
    from multishiftseg_amd import m2f_targets
    maps = R.rand_maps(B, H, W, 4)
    images, targets = _run(D, maps, _draw(D, 5))
    assert images.shape == (2 * B, 3) + CROP and targets.shape == (2 * B,) + CROP and targets.dtype == torch.int64
    assert int(targets.min()) >= 0 and int(targets.max()) <= 255
    t = m2f_targets.prepare_targets(targets)
    assert len(t) == 2 * B
    torch.cuda.synchronize()
