"""Test oracle of the Mask2Former input path (multishiftseg_amd/m2f_datapath.py): a stock-torch CPU restatement of every
op of the chain and of the draw order, written from the formulas of torchvision 0.16.2's tensor code paths (neither
torchvision nor the reference's img_utils can be imported where the tests run). Every float op takes `dtype`, so that it runs
in float32 and in float64: the device is held to max|device - f64| <= max(8 e, 2^-20) with e = max|f32 - f64| of the same op
on the same input (bound()). Working set as on the device: x [N, 3, H, W] in [0, 1], m uint8 [N, H, W]."""
import math

import numpy as np
import torch
import torch.nn.functional as F

CHAIN = (("ToTensor", 1.0), ("ColorJitter", 0.5), ("GaussianBlur", 0.5), ("RandSharpness", 0.5), ("AutoContrast", 0.5),
         ("Equalize", 0.5), ("RandResize", 0.5), ("RandRotate", 0.5), ("RandHorizontalFlip", 0.5), ("RandVerticalFlip", 0.5),
         ("RandCrop", 1.0), ("Normalize", 1.0))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FLOOR = 2.0 ** -20
EXACT = ("ToTensor", "RandHorizontalFlip", "RandVerticalFlip", "RandCrop", "Normalize")


def bound(op, *args, **kw):
    """(float64 result, allowed max |device - float64|) of a float op: max(8 e, 2^-20), e = max |f32 - f64| on this input."""
    r32, r64 = op(*args, dtype=torch.float32, **kw), op(*args, dtype=torch.float64, **kw)
    e = float((r32.double() - r64).abs().max())
    return r64, max(8.0 * e, FLOOR), e


# ---- load ---------------------------------------------------------------------------------------------------------------------
def load(img, gen, tgt, gen_tgt, p):
    """uint8 [H,W,3] x 2, uint8 [H,W] x 2 -> (x float32 [2,3,H,W], m uint8 [2,H,W]); exact."""
    a, g = img.numpy(), gen.numpy()
    if p is not None:
        g = (p * a + (1 - p) * g).astype(np.uint8)
    x = torch.stack([torch.from_numpy(a), torch.from_numpy(g)]).permute(0, 3, 1, 2).to(torch.float32) / 255.0
    return x.contiguous(), torch.stack([tgt, gen_tgt])


# ---- colour -------------------------------------------------------------------------------------------------------------------
def blend(a, b, r):
    return (r * a + (1.0 - r) * b).clamp(0, 1)


def gray(x):
    return (0.2989 * x[:, 0] + 0.587 * x[:, 1] + 0.114 * x[:, 2]).unsqueeze(1)


def brightness(x, f, dtype=torch.float32):
    x = x.to(dtype)
    return blend(x, torch.zeros_like(x), f)


def contrast(x, f, dtype=torch.float32):
    x = x.to(dtype)
    return blend(x, gray(x).mean(dim=(-3, -2, -1), keepdim=True), f)


def saturation(x, f, dtype=torch.float32):
    x = x.to(dtype)
    return blend(x, gray(x), f)


def hue(x, f, dtype=torch.float32):
    x = x.to(dtype)
    r, g, b = x.unbind(1)
    maxc, minc = x.max(dim=1).values, x.min(dim=1).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    div = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    h = (h + f) % 1.0
    v = maxc
    i = torch.floor(h * 6.0)
    fr = h * 6.0 - i
    i = i.to(torch.int64) % 6
    p = (v * (1.0 - s)).clamp(0, 1)
    q = (v * (1.0 - fr * s)).clamp(0, 1)
    t = (v * (1.0 - (1.0 - fr) * s)).clamp(0, 1)
    table = torch.stack([torch.stack([v, q, p, p, t, v]), torch.stack([t, v, v, q, p, p]), torch.stack([p, p, t, v, v, q])])   # [3,6,N,H,W]
    return torch.gather(table, 1, i.expand(3, 1, *i.shape)).squeeze(1).permute(1, 0, 2, 3)


COLOUR = (brightness, contrast, saturation, hue)


def color_jitter(x, perm, factors, dtype=torch.float32):
    x = x.to(dtype)
    for i in perm:
        x = COLOUR[i](x, factors[i], dtype=dtype)
    return x


def autocontrast(x, dtype=torch.float32):
    x = x.to(dtype)
    lo, hi = x.amin(dim=(-2, -1), keepdim=True), x.amax(dim=(-2, -1), keepdim=True)
    scale = 1.0 / (hi - lo)
    bad = ~torch.isfinite(scale)
    lo = torch.where(bad, torch.zeros_like(lo), lo)
    scale = torch.where(bad, torch.ones_like(scale), scale)
    return ((x - lo) * scale).clamp(0, 1)


# ---- filters --------------------------------------------------------------------------------------------------------------------
def gaussian_kernel1d(sigma):
    t = torch.linspace(-4.0, 4.0, steps=9)
    pdf = torch.exp(-0.5 * (t / sigma).pow(2))
    return pdf / pdf.sum()                         # float32 whatever the op's dtype: the weights are part of the specification


def gaussian_blur(x, sigma, dtype=torch.float32):
    x = x.to(dtype)
    k1 = gaussian_kernel1d(sigma).to(dtype)
    k2 = (k1[:, None] * k1[None, :]).expand(3, 1, 9, 9)
    return F.conv2d(F.pad(x, (4, 4, 4, 4), mode="reflect"), k2, groups=3)


def sharpness(x, f, dtype=torch.float32):
    x = x.to(dtype)
    if x.shape[-2] <= 2 or x.shape[-1] <= 2:
        return x
    k = torch.ones(3, 3, dtype=dtype)
    k[1, 1] = 5.0
    k = (k / k.sum()).expand(3, 1, 3, 3)
    d = x.clone()
    d[..., 1:-1, 1:-1] = F.conv2d(x, k, groups=3)
    return blend(x, d, f)


def equalize(x, dtype=torch.float32):
    """Integer arithmetic; the result is float32(u) / 255 whatever dtype says (it is exact on byte-valued input)."""
    u = (x.to(torch.float32) * 255).to(torch.uint8)
    out = u.clone()
    for n in range(u.shape[0]):
        for c in range(3):
            ch = u[n, c].to(torch.int64)
            hist = torch.bincount(ch.reshape(-1), minlength=256)
            nz = hist[hist != 0]
            step = int(nz[:-1].sum()) // 255
            if step == 0:
                continue
            lut = (torch.cumsum(hist, 0) + step // 2) // step
            lut = F.pad(lut, [1, 0])[:-1].clamp(0, 255)
            out[n, c] = lut[ch].to(torch.uint8)
    return (out.to(torch.float32) / 255).to(dtype)


# ---- warps ----------------------------------------------------------------------------------------------------------------------
def resize(x, size, dtype=torch.float32):
    return F.interpolate(x.to(dtype), size=size, mode="bilinear", align_corners=False, antialias=False)


def resize_mask(m, size):
    return F.interpolate(m[:, None].to(torch.float32), size=size, mode="nearest")[:, 0].to(torch.uint8)


def rotate_grid(H, W, angle, dtype):
    r = math.radians(-angle)
    theta = torch.tensor([[math.cos(r), math.sin(r), 0.0], [-math.sin(r), math.cos(r), 0.0]], dtype=dtype)
    xg = torch.linspace(-W * 0.5 + 0.5, W * 0.5 - 0.5, W, dtype=dtype)
    yg = torch.linspace(-H * 0.5 + 0.5, H * 0.5 - 0.5, H, dtype=dtype)
    base = torch.stack([xg[None, :].expand(H, W), yg[:, None].expand(H, W), torch.ones(H, W, dtype=dtype)], dim=-1)
    resc = theta.t() / torch.tensor([0.5 * W, 0.5 * H], dtype=dtype)
    return (base.view(1, H * W, 3) @ resc[None]).view(1, H, W, 2)


def rotate(x, angle, dtype=torch.float32):
    N, _, H, W = x.shape
    grid = rotate_grid(H, W, angle, dtype).expand(N, H, W, 2)
    return F.grid_sample(x.to(dtype), grid, mode="bilinear", padding_mode="zeros", align_corners=False)


def rotate_mask(m, angle, dtype=torch.float32):
    N, H, W = m.shape
    grid = rotate_grid(H, W, angle, dtype).expand(N, H, W, 2)
    return F.grid_sample(m[:, None].to(dtype), grid, mode="nearest", padding_mode="zeros", align_corners=False)[:, 0].to(torch.uint8)


def rotate_mask_decided(H, W, angle, eps=1e-3):
    """bool [H, W]: the pixels whose float64 source coordinate is at least eps away from a rounding boundary in x and y."""
    g = rotate_grid(H, W, angle, torch.float64)[0]
    ix, iy = ((g[..., 0] + 1) * W - 1) / 2, ((g[..., 1] + 1) * H - 1) / 2
    fx, fy = ix - torch.floor(ix), iy - torch.floor(iy)
    return ((fx - 0.5).abs() >= eps) & ((fy - 0.5).abs() >= eps)


# ---- flips, crop, Normalize, paste -----------------------------------------------------------------------------------------------
def window(x, m, hflip=False, vflip=False, top=0, left=0, size=None):
    if hflip:
        x, m = x.flip(-1), m.flip(-1)
    if vflip:
        x, m = x.flip(-2), m.flip(-2)
    h, w = size if size is not None else x.shape[-2:]
    return x[..., top:top + h, left:left + w].contiguous(), m[..., top:top + h, left:left + w].contiguous()


def normalize(x, mean=MEAN, std=STD):
    mt = torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)
    st = torch.tensor(std, dtype=torch.float32).view(1, 3, 1, 1)
    return (x.to(torch.float32) - mt) / st


def paste(img, tgt, obj_img, obj_mask, geom, mean=MEAN, std=STD):
    """img float32 [3,h,w] normalised, tgt int64 [h,w]; the object region (y1, x1, bh, bw) goes to (h0, w0) wherever the
    mask is neither 0 nor 255; object pixels: float32(v / 255) then - mean, / std in float64."""
    y1, x1, bh, bw, h0, w0 = geom
    img, tgt = img.clone(), tgt.clone()
    if bh <= 0 or bw <= 0:
        return img, tgt
    om = torch.as_tensor(obj_mask)[y1:y1 + bh, x1:x1 + bw]
    oi = torch.as_tensor(obj_img, dtype=torch.float32)[y1:y1 + bh, x1:x1 + bw]
    v = (oi / 255.0).to(torch.float64)
    v = ((v - torch.tensor(mean, dtype=torch.float64)) / torch.tensor(std, dtype=torch.float64)).to(torch.float32).permute(2, 0, 1)
    sel = (om != 0) & (om != 255)
    reg_i, reg_t = img[:, h0:h0 + bh, w0:w0 + bw], tgt[h0:h0 + bh, w0:w0 + bw]
    reg_i[:, sel] = v[:, sel]
    reg_t[sel] = om[sel].to(torch.int64)
    return img, tgt


# ---- the chain, one entry at a time ----------------------------------------------------------------------------------------------
def apply_entry(x, m, e, crop_size, dtype=torch.float32):
    """One applied chain entry (a dict of draw_restated / draw_m2f_sample_params) on (x, m) -> (x, m)."""
    name = e["name"]
    if name == "ColorJitter":
        return color_jitter(x, e["perm"], (e["brightness"], e["contrast"], e["saturation"], e["hue"]), dtype=dtype), m
    if name == "GaussianBlur":
        return gaussian_blur(x, e["sigma"], dtype=dtype), m
    if name == "RandSharpness":
        return sharpness(x, e["factor"], dtype=dtype), m
    if name == "AutoContrast":
        return autocontrast(x, dtype=dtype), m
    if name == "Equalize":
        return equalize(x, dtype=dtype), m
    if name == "RandResize":
        return resize(x, e["size"], dtype=dtype), resize_mask(m, e["size"])
    if name == "RandRotate":
        return rotate(x, e["angle"], dtype=dtype), rotate_mask(m, e["angle"], dtype=dtype)
    if name == "RandHorizontalFlip":
        return window(x, m, hflip=True)
    if name == "RandVerticalFlip":
        return window(x, m, vflip=True)
    if name == "RandCrop":
        return window(x, m, top=e["top"], left=e["left"], size=crop_size)
    if name == "Normalize":
        return normalize(x), m
    assert name == "ToTensor", name
    return x, m


# ---- the draw order, restated ------------------------------------------------------------------------------------------------------
def _bbox(mask):
    sel = (np.asarray(mask) != 0) & (np.asarray(mask) != 255)
    ys, xs = np.nonzero(sel)
    if ys.size == 0:
        return 0, 0, 0, 0
    return int(ys.min()), int(xs.min()), int(ys.max()) + 1, int(xs.max()) + 1


def draw_restated(H, W, crop_size, mixup, objects, scaled_object, rng, chain=CHAIN, scales=(0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0)):
    """The sample's draws in the order the reference's code makes them: `rng` for Compose and the img_utils transforms,
    torch's default generator for torchvision's ColorJitter and GaussianBlur."""
    out = {"p": None}
    if mixup:
        out["p"] = min(rng.random(), 0.3)
    size = [H, W]
    entries = []
    for name, prob in chain:
        take = rng.random() < prob
        if not take:
            continue
        e = {"name": name}
        if name == "ColorJitter":
            e["perm"] = [int(v) for v in torch.randperm(4)]
            for key, (lo, hi) in (("brightness", (max(0, 1 - 0.8), 1 + 0.8)), ("contrast", (max(0, 1 - 0.8), 1 + 0.8)),
                                  ("saturation", (max(0, 1 - 0.8), 1 + 0.8)), ("hue", (-0.2, 0.2))):
                e[key] = float(torch.empty(1).uniform_(lo, hi))
        if name == "GaussianBlur":
            e["sigma"] = torch.empty(1).uniform_(0.1, 5.0).item()
        if name == "RandSharpness":
            e["factor"] = rng.random() * 2
        if name == "RandResize":
            e["scale"] = rng.choice([0.7, 0.8, 0.9, 1.0])
            size = [int(size[0] * e["scale"]), int(size[1] * e["scale"])]
            e["size"] = tuple(size)
        if name == "RandRotate":
            e["angle"] = rng.random() * 20 - 10
        if name == "RandCrop":
            e["top"] = rng.randint(0, size[0] - crop_size[0])
            e["left"] = rng.randint(0, size[1] - crop_size[1])
            out["top"], out["left"] = e["top"], e["left"]
        entries.append(e)
    out["entries"], out["size"] = entries, tuple(size)
    if objects:
        obj = objects[rng.randint(0, len(objects) - 1)]
        o_img, o_mask = scaled_object(obj, rng.choice(list(scales)))
        y1, x1, y2, x2 = _bbox(o_mask)
        h0 = rng.randint(0, crop_size[0] - (y2 - y1))
        w0 = rng.randint(0, crop_size[1] - (x2 - x1))
        out.update(obj_img=o_img, obj_mask=o_mask, geom=(y1, x1, y2 - y1, x2 - x1, h0, w0))
    return out


# ---- inputs shared by the CPU and GPU tests ------------------------------------------------------------------------------------
SHAPES = ((23, 37), (37, 53), (64, 96), (70, 151))      # the last: > 1 workgroup in each grid dimension, H W not a multiple of 4
ANGLES = (-10.0, -3.7, 0.0, 0.001, 5.25, 10.0)


def rand_stack(H, W, seed=0, N=2):
    """x float32 [N,3,H,W] in [0,1] with the cases the colour ops branch on -- gray pixels, channel-maximum ties, exact 0 and
    1 -- and m uint8 [N,H,W]."""
    g = torch.Generator().manual_seed(seed * 7919 + H * 131 + W)
    x = torch.rand(N, 3, H, W, generator=g)
    k = torch.rand(N, H, W, generator=g)
    x[:, 1] = torch.where(k < 0.1, x[:, 0], x[:, 1])                # r == g ties
    x[:, 2] = torch.where(k < 0.05, x[:, 0], x[:, 2])               # gray pixels
    x[:, 2] = torch.where((k > 0.1) & (k < 0.15), x[:, 1], x[:, 2])  # g == b ties
    x = torch.where(torch.rand(N, 3, H, W, generator=g) < 0.03, torch.zeros(()), x)
    x = torch.where(torch.rand(N, 3, H, W, generator=g) < 0.03, torch.ones(()), x)
    m = torch.randint(0, 256, (N, H, W), generator=g, dtype=torch.uint8)
    return x.contiguous(), m


def rand_bytes(H, W, seed=0, N=2):
    x, m = rand_stack(H, W, seed, N)
    return ((x * 255).to(torch.uint8).to(torch.float32) / 255).contiguous(), m


def rand_maps(B, H, W, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    gen = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    tgt = torch.randint(0, 19, (B, H, W), generator=g, dtype=torch.uint8)
    gtg = torch.randint(0, 256, (B, H, W), generator=g, dtype=torch.uint8)
    return img, gen, tgt, gtg


def rand_objects(n=3, seed=0):
    """Candidates for the paste: (image float32 [oh,ow,3] in 0..255, mask uint8 [oh,ow] with 0, 255 and a class id)."""
    r = np.random.default_rng(seed)
    out = []
    for k in range(n):
        oh, ow = 9 + 2 * k, 12 + k
        mask = np.zeros((oh, ow), np.uint8)
        mask[2:oh - 1, 1:ow - 2] = 254
        mask[3, 3] = 255
        mask[4, 4] = 0
        out.append((r.uniform(0, 255, (oh, ow, 3)).astype(np.float32), mask))
    return out


def scaled_object(obj, scale):
    """Stands in for the caller's cv2 rescale: crops the object to the scale's share of its rows (any deterministic map will do)."""
    img, mask = obj
    rows = max(5, int(img.shape[0] * (0.5 + 0.5 * scale)))
    return img[:rows], mask[:rows]
