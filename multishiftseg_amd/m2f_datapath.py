"""On-device input path of the Mask2Former trainer (datapath.py is the DeepLab trainer's).

train_m2f.py:48-61 builds every sample through a chain of twelve transforms (lib/utils/img_utils.py), each drawn with its
own probability and applied jointly to image, label map, generated image and generated label map; DiverseCityscapes
mixes the generated image with the original before (lib/dataset/cityscapes.py:160-164) and pastes a COCO object after it
(cityscapes.py:168-169). On four CPU workers that delivers a few samples per second.

Here the decoded uint8 maps live in HBM, the random DECISIONS are drawn on the host in the reference's order
(draw_m2f_sample_params) and the arithmetic runs in the HIP kernels of libmss_aug.so (include/mss_aug_hip.h, csrc/aug*.hip).
Sizes differ per sample after RandResize, so a sample is processed on its own: its working set is x float32 [2, 3, Hs, Ws]
(image, generated image: the reference's own stack of two) and m uint8 [2, Hs, Ws]; the last kernel writes straight into the
sample's two slots of the batch. Every stage is also callable alone (the functions below), which is what the tests do.

QUIRK kept on purpose: the reference rotates without a `fill`, so rotated-in corners are black and CLASS 0 in the label map.

The pasted COCO object comes either from the caller, already rescaled (scaled_object), or from a resident
object_bank.ObjectBank: draw_m2f_sample_params then hands on pick=(index, scale) and make_m2f_pair_batch(..., bank=bank) rescales
and cuts the objects of the whole batch with one launch; a sample takes its slot.

There is no CPU path: a CPU tensor raises. File decoding stays the caller's.
"""
import ctypes
import math
import random as _random

import torch

from . import _lib_aug as A
from ._lib_aug import call, ptr
from .datapath import MEAN, STD, bank_objects, draw_sample_params

# train_m2f.py:48-61
M2F_CHAIN = (("ToTensor", 1.0), ("ColorJitter", 0.5), ("GaussianBlur", 0.5), ("RandSharpness", 0.5), ("AutoContrast", 0.5),
             ("Equalize", 0.5), ("RandResize", 0.5), ("RandRotate", 0.5), ("RandHorizontalFlip", 0.5), ("RandVerticalFlip", 0.5),
             ("RandCrop", 1.0), ("Normalize", 1.0))
RESIZE_SCALES = [0.7, 0.8, 0.9, 1.0]                 # train_m2f.py:55
JITTER = (0.8, 0.8, 0.8, 0.2)                        # img_utils.py:138: brightness, contrast, saturation, hue
BLUR_SIGMA = (0.1, 5.0)                              # img_utils.py:144
_KIND = (A.OP_BRIGHTNESS, A.OP_CONTRAST, A.OP_SATURATION, A.OP_HUE)      # ColorJitter's fn_idx -> op
_NEEDS_STATS = (A.OP_CONTRAST, A.OP_AUTOCONTRAST)


class _ReplayCrop:
    """What datapath.draw_sample_params sees as `rng` when only its paste draws are wanted: the first two randint calls (its
    crop corner) hand back the corner this chain has drawn already and consume nothing; everything else is the real rng."""

    def __init__(self, rng, top, left):
        self._rng, self._replay = rng, [top, left]

    def randint(self, a, b):
        return self._replay.pop(0) if self._replay else self._rng.randint(a, b)

    def __getattr__(self, name):
        return getattr(self._rng, name)


def draw_m2f_sample_params(H, W, crop_size, mixup=True, objects=None, scaled_object=None, rng=_random, chain=M2F_CHAIN):
    """Random decisions of ONE sample in the reference's order. Returns {"p", "entries", "size", "top", "left"} and, with
    objects, obj_img / obj_mask / geom (pick / geom when objects is a bank) as datapath.draw_sample_params. "entries" lists the APPLIED chain entries in order,
    each a dict with "name" and its own draws. ColorJitter and GaussianBlur read torch's default CPU generator, as
    torchvision does; everything else reads `rng`."""
    p = min(rng.random(), 0.3) if mixup else None                              # cityscapes.py:161
    Hs, Ws = H, W
    entries = []
    top = left = None
    for name, prob in chain:
        if not rng.random() < prob:                                            # Compose.__call__, img_utils.py:47
            continue
        e = {"name": name}
        if name == "ColorJitter":                                              # torchvision ColorJitter.get_params
            e["perm"] = torch.randperm(4).tolist()
            b, c, s, h = JITTER
            e["brightness"] = float(torch.empty(1).uniform_(max(0, 1 - b), 1 + b))
            e["contrast"] = float(torch.empty(1).uniform_(max(0, 1 - c), 1 + c))
            e["saturation"] = float(torch.empty(1).uniform_(max(0, 1 - s), 1 + s))
            e["hue"] = float(torch.empty(1).uniform_(-h, h))
        elif name == "GaussianBlur":                                           # torchvision GaussianBlur.get_params
            e["sigma"] = torch.empty(1).uniform_(BLUR_SIGMA[0], BLUR_SIGMA[1]).item()
        elif name == "RandSharpness":
            e["factor"] = rng.random() * 2                                     # img_utils.py:195
        elif name == "RandResize":
            scale = rng.choice(RESIZE_SCALES)                                  # img_utils.py:241-242
            Hs, Ws = int(Hs * scale), int(Ws * scale)
            e["scale"], e["size"] = scale, (Hs, Ws)
        elif name == "RandRotate":
            e["angle"] = rng.random() * 20 - 10                                # img_utils.py:322
        elif name == "RandCrop":
            if Hs < crop_size[0] or Ws < crop_size[1]:
                # img_utils.py:254-258 resizes the image alone here and then fails to stack it with the generated one
                raise ValueError(f"the resized sample ({Hs} x {Ws}) is smaller than the crop {tuple(crop_size)}")
            top = e["top"] = rng.randint(0, Hs - crop_size[0])                 # img_utils.py:256
            left = e["left"] = rng.randint(0, Ws - crop_size[1])               # img_utils.py:257
        entries.append(e)
    out = {"p": p, "entries": entries, "size": (Hs, Ws), "top": top, "left": left}
    if objects:
        if top is None:
            raise ValueError("the paste needs the crop: the chain applied no RandCrop")
        paste = draw_sample_params(Hs, Ws, crop_size, False, objects, scaled_object, _ReplayCrop(rng, top, left))
        if "pick" in paste:         # objects is a bank: the object tensors come from bank.rescale in make_m2f_pair_batch
            out.update(pick=paste["pick"], geom=paste["geom"])
        else:
            out.update(obj_img=paste["obj_img"], obj_mask=paste["obj_mask"], geom=paste["geom"])
    return out


# ---- the stages, each callable alone ---------------------------------------------------------------------------------------

def _gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("multishiftseg_amd.m2f_datapath runs on an MI355X only; there is no CPU path")


def _stack(x, m=None):
    _gpu(x, m)
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or not x.is_contiguous():
        raise TypeError("x must be a contiguous float32 [N, 3, H, W] tensor")
    if m is not None and (m.dtype != torch.uint8 or m.shape != (x.shape[0],) + x.shape[2:] or not m.is_contiguous()):
        raise TypeError("m must be a contiguous uint8 [N, H, W] tensor")
    return x.shape[0], x.shape[2], x.shape[3]


def load_pair(img, gen, tgt, gen_tgt, p=None):
    """uint8 [H,W,3] x 2, uint8 [H,W] x 2 -> x float32 [2,3,H,W], m uint8 [2,H,W]: mixup (p not None) and ToTensor."""
    _gpu(img, gen, tgt, gen_tgt)
    for t in (img, gen, tgt, gen_tgt):
        if t.dtype != torch.uint8 or not t.is_contiguous():
            raise TypeError("pre-decoded maps must be contiguous uint8 tensors")
    H, W, _ = img.shape
    x = torch.empty((2, 3, H, W), device=img.device, dtype=torch.float32)
    m = torch.zeros((2, H, W), device=img.device, dtype=torch.uint8)
    call("mss_aug_load_f32", ptr(img), ptr(gen), ptr(tgt), ptr(gen_tgt), H, W, int(p is not None), float(p or 0.0), ptr(x), ptr(m))
    return x, m


def image_stats(x):
    """float32 [N, 8]: mean of gray, then (min, max) of r, g, b per image. Fixed-order reduction: reproducible bits."""
    N, H, W = _stack(x)
    ws = torch.empty((N * A.value("mss_aug_stats_ws_doubles", H, W),), device=x.device, dtype=torch.float64)
    stats = torch.empty((N, 8), device=x.device, dtype=torch.float32)
    call("mss_aug_stats_f32", ptr(x), N, H, W, ptr(ws), ptr(stats))
    return stats


def pointwise(x, ops):
    """Apply [(kind, factor), ...] to x in place, in as few passes as the ops allow: a run is cut where an op needs the
    statistics of the current state (contrast's mean, autocontrast's min / max) or after eight ops."""
    N, H, W = _stack(x)
    run, stats = [], None

    def flush():
        if run:
            po = A.MssAugPointOps(n=len(run))
            for k, (kind, f) in enumerate(run):
                po.kind[k], po.factor[k] = kind, f
            call("mss_aug_pointwise_f32", ptr(x), N, H, W, ctypes.byref(po), ptr(stats))
            run.clear()
    for kind, f in ops:
        if kind in _NEEDS_STATS or len(run) == A.MSS_AUG_MAX_OPS:
            flush()
        if kind in _NEEDS_STATS:
            stats = image_stats(x)
        run.append((kind, float(f)))
    flush()
    return x


def color_jitter(x, perm, brightness, contrast, saturation, hue):
    factors = (brightness, contrast, saturation, hue)
    return pointwise(x, [(_KIND[i], factors[i]) for i in perm])


def autocontrast(x):
    return pointwise(x, [(A.OP_AUTOCONTRAST, 0.0)])


def gaussian_kernel1d(sigma):
    """torchvision's _get_gaussian_kernel1d(9, sigma) in float32, on the host."""
    t = torch.linspace(-4.0, 4.0, steps=9)
    pdf = torch.exp(-0.5 * (t / sigma).pow(2))
    return pdf / pdf.sum()


def gaussian_blur(x, sigma):
    N, H, W = _stack(x)
    k9 = (ctypes.c_float * 9)(*gaussian_kernel1d(sigma).tolist())
    y = torch.empty_like(x)
    call("mss_aug_blur9_f32", ptr(x), ptr(y), N, H, W, ctypes.cast(k9, ctypes.c_void_p))
    return y


def sharpness(x, factor):
    N, H, W = _stack(x)
    y = torch.empty_like(x)
    call("mss_aug_sharpness_f32", ptr(x), ptr(y), N, H, W, float(factor))
    return y


def equalize(x):
    """In place: quantise to bytes, equalise every image channel through its own look-up table, back to float / 255."""
    N, H, W = _stack(x)
    ws = torch.zeros((N * 3 * 512,), device=x.device, dtype=torch.int32)
    call("mss_aug_equalize_f32", ptr(x), N, H, W, ptr(ws))
    return x


def resize(x, m, size):
    N, H, W = _stack(x, m)
    OH, OW = size
    y = torch.empty((N, 3, OH, OW), device=x.device, dtype=torch.float32)
    mo = torch.zeros((N, OH, OW), device=x.device, dtype=torch.uint8)
    call("mss_aug_resize_f32", ptr(x), ptr(m), N, H, W, OH, OW, ptr(y), ptr(mo))
    return y, mo


def rotate(x, m, angle):
    """Rotate by `angle` degrees about the centre (torchvision F.rotate without expand / fill): label 0 rotates in."""
    N, H, W = _stack(x, m)
    r = math.radians(-angle)
    c, s = torch.tensor([math.cos(r), math.sin(r)], dtype=torch.float32).tolist()     # theta as torch.tensor(matrix, float32)
    y = torch.empty_like(x)
    mo = torch.zeros_like(m)
    call("mss_aug_rotate_f32", ptr(x), ptr(m), N, H, W, c, s, ptr(y), ptr(mo))
    return y, mo


def window(x, m, hflip=False, vflip=False, top=0, left=0, size=None):
    """Flips, then the crop window [top, top + h) x [left, left + w) of the flipped maps. Exact copies."""
    N, H, W = _stack(x, m)
    h, w = size if size is not None else (H, W)
    y = torch.empty((N, 3, h, w), device=x.device, dtype=torch.float32)
    mo = torch.zeros((N, h, w), device=x.device, dtype=torch.uint8)
    call("mss_aug_window_f32", ptr(x), ptr(m), N, H, W, int(hflip), int(vflip), top, left, h, w, ptr(y), ptr(mo))
    return y, mo


def finish(x, m, out_img, out_tgt, b, hflip=False, vflip=False, top=0, left=0, size=None, mean=MEAN, std=STD, obj_img=None,
           obj_mask=None, geom=None):
    """Window, Normalize, paste (geom = (y1, x1, bh, bw, h0, w0), obj_img float32 [oh,ow,3], obj_mask uint8 [oh,ow] on the
    device) and the batch layout: image 0 -> slot b, image 1 -> slot B + b of out_img [2B,3,h,w] / out_tgt int64 [2B,h,w]."""
    N, H, W = _stack(x, m)
    _gpu(out_img, out_tgt, obj_img, obj_mask)
    h, w = size if size is not None else (H, W)
    B = out_img.shape[0] // 2
    if N != 2 or out_img.dtype != torch.float32 or out_tgt.dtype != torch.int64 or tuple(out_img.shape) != (2 * B, 3, h, w) \
            or tuple(out_tgt.shape) != (2 * B, h, w) or not out_img.is_contiguous() or not out_tgt.is_contiguous():
        raise TypeError("finish writes a stack of two into float32 [2B,3,h,w] / int64 [2B,h,w] batches")
    mean3 = (ctypes.c_double * 3)(*[float(v) for v in mean])
    std3 = (ctypes.c_double * 3)(*[float(v) for v in std])
    g6, OH, OW = None, 0, 0
    if geom is not None:
        if obj_img.dtype != torch.float32 or obj_mask.dtype != torch.uint8 or not obj_img.is_contiguous() or not obj_mask.is_contiguous():
            raise TypeError("the object is a contiguous float32 [oh,ow,3] image and a uint8 [oh,ow] mask")
        OH, OW = obj_mask.shape
        g6 = ctypes.cast((ctypes.c_int * 6)(*[int(v) for v in geom]), ctypes.c_void_p)
    call("mss_aug_finish_f32", ptr(x), ptr(m), H, W, int(hflip), int(vflip), top, left, h, w, ctypes.cast(mean3, ctypes.c_void_p),
         ctypes.cast(std3, ctypes.c_void_p), ptr(obj_img), ptr(obj_mask), OH, OW, g6, B, b, ptr(out_img), ptr(out_tgt))


# ---- the chain ---------------------------------------------------------------------------------------------------------------

def _sample(img, gen, tgt, gen_tgt, crop_size, prm, b, out_img, out_tgt, mean, std, trace, picked=None):
    x, m = load_pair(img, gen, tgt, gen_tgt, prm["p"])
    names = [e["name"] for e in prm["entries"]]
    if names[:1] != ["ToTensor"] or names[-2:] != ["RandCrop", "Normalize"]:
        raise ValueError("the chain must apply ToTensor first and RandCrop, Normalize last")
    hflip = vflip = False
    pending = []                    # point-wise ops not launched yet: consecutive colour entries share one pass

    def note(name):
        if trace is not None:
            trace.append((name, x.clone(), m.clone()))
    for e in prm["entries"]:
        name = e["name"]
        if name == "ColorJitter":
            f = (e["brightness"], e["contrast"], e["saturation"], e["hue"])
            pending += [(_KIND[i], f[i]) for i in e["perm"]]
        elif name == "AutoContrast":
            pending.append((A.OP_AUTOCONTRAST, 0.0))
        if pending and (trace is not None or name not in ("ColorJitter", "AutoContrast")):
            pointwise(x, pending)
            pending = []
        if name == "GaussianBlur":
            x = gaussian_blur(x, e["sigma"])
        elif name == "RandSharpness":
            x = sharpness(x, e["factor"])
        elif name == "Equalize":
            equalize(x)
        elif name == "RandResize":
            x, m = resize(x, m, e["size"])
        elif name == "RandRotate":
            x, m = rotate(x, m, e["angle"])
        elif name == "RandHorizontalFlip":
            hflip = True
            if trace is not None:
                x, m = window(x, m, hflip=True)
        elif name == "RandVerticalFlip":
            vflip = True
            if trace is not None:
                x, m = window(x, m, vflip=True)
        elif name == "RandCrop":
            if trace is not None:
                x, m = window(x, m, top=e["top"], left=e["left"], size=crop_size)
        elif name == "Normalize":
            break
        note(name)
    paste = dict(obj_img=None, obj_mask=None, geom=None)
    if picked is not None:          # slot b of the batch's bank.rescale
        paste = dict(obj_img=picked[0][b], obj_mask=picked[1][b], geom=prm["geom"])
    elif "geom" in prm:
        dev = x.device
        paste = dict(obj_img=torch.as_tensor(prm["obj_img"], dtype=torch.float32).contiguous().to(dev),
                     obj_mask=torch.as_tensor(prm["obj_mask"], dtype=torch.uint8).contiguous().to(dev), geom=prm["geom"])
    if trace is not None:           # flips and crop are done: Normalize alone for the trace, then Normalize + paste into the batch
        t_img = torch.empty((2, 3) + tuple(crop_size), device=x.device, dtype=torch.float32)
        t_tgt = torch.zeros((2,) + tuple(crop_size), device=x.device, dtype=torch.int64)
        finish(x, m, t_img, t_tgt, 0, mean=mean, std=std)
        trace.append(("Normalize", t_img, m.clone()))
        finish(x, m, out_img, out_tgt, b, mean=mean, std=std, **paste)
    else:
        finish(x, m, out_img, out_tgt, b, hflip=hflip, vflip=vflip, top=prm["top"], left=prm["left"], size=crop_size, mean=mean, std=std,
               **paste)


def make_m2f_pair_batch(img, gen, tgt, gen_tgt, crop_size, params, mean=MEAN, std=STD, trace=None, bank=None):
    """img / gen: uint8 [B,H,W,3] device tensors, tgt / gen_tgt: uint8 [B,H,W]; params: one dict per sample as returned by
    draw_m2f_sample_params; bank: the object_bank.ObjectBank the sets were drawn from, when they carry `pick`. Returns (images float32 [2B,3,h,w], targets int64 [2B,h,w]), originals first
    (train_m2f.py:430-433). trace: a list that receives (stage name, x clone, m clone) after every applied entry of every
    sample (the stages then run one by one instead of fused; the results are the same bits)."""
    _gpu(img, gen, tgt, gen_tgt)
    for t in (img, gen, tgt, gen_tgt):
        if t.dtype != torch.uint8 or not t.is_contiguous():
            raise TypeError("pre-decoded maps must be contiguous uint8 tensors")
    B, H, W, _ = img.shape
    h, w = crop_size
    if len(params) != B:
        raise ValueError(f"{len(params)} parameter sets for a batch of {B}")
    out_img = torch.empty((2 * B, 3, h, w), device=img.device, dtype=torch.float32)
    out_tgt = torch.zeros((2 * B, h, w), device=img.device, dtype=torch.int64)
    picked = bank_objects(params, bank)
    for b, prm in enumerate(params):
        _sample(img[b], gen[b], tgt[b], gen_tgt[b], (h, w), prm, b, out_img, out_tgt, mean, std, trace, picked)
    return out_img, out_tgt
