"""numpy restatement of the object bank's arithmetic: cv2.resize as the reference's random_scale calls it,
written out from the rules alone -- INTER_NEAREST for the mask, INTER_LINEAR for the image, the valid-pixel bounding box.

    inv = (double)dst / src, scale = 1.0 / inv                                   per axis, all in float64
    nearest:  s = min(floor(d * scale), src - 1)
    linear:   f = float32((d + 0.5) * scale - 0.5); s = floor(f); f = f - float32(s)
              s < 0 -> s = 0, f = 0;   s >= src - 1 -> s = src - 1, f = 0 (second tap = the same pixel)
              a1 = f, a0 = float32(1) - f; rows alike (b0, b1)
              h   = fl(fl(S[r, s] a0) + fl(S[r, s1] a1))                         horizontal pass first
              dst = fl(fl(h[sy] b0) + fl(h[sy1] b1))                             then the vertical pass
"""
import numpy as np

F32 = np.float32


def scaled_size(H, W, scale):
    """img_utils.py:347-348 in Python float arithmetic."""
    return int(H * scale), int(W * scale)


def scale_factor(src, dst):
    inv = np.float64(dst) / np.float64(src)
    return np.float64(1.0) / inv


def nearest_index(src, dst):
    """int64 [dst]: the source index of every destination index."""
    d = np.arange(dst, dtype=np.float64)
    return np.minimum(np.floor(d * scale_factor(src, dst)).astype(np.int64), src - 1)


def linear_taps(src, dst):
    """(s0 int64 [dst], s1 int64 [dst], f float32 [dst]): taps and the weight of the second one."""
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale_factor(src, dst) - 0.5).astype(F32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(F32)).astype(F32)
    low, high = s < 0, s >= src - 1
    s = np.where(low, 0, s)
    s = np.where(high, src - 1, s)
    f = np.where(low | high, F32(0), f).astype(F32)
    return s, np.minimum(s + 1, src - 1), f


def fl(x):
    """Rounding to float32, spelled out at every operation of the float32 form."""
    return np.asarray(x, dtype=F32)


def linear(img, sh, sw):
    """img uint8 (or integer-valued float) [H, W, C] -> float32 [sh, sw, C], one defined sequence of float32 operations."""
    S = fl(img)
    H, W = S.shape[:2]
    x0, x1, fx = linear_taps(W, sw)
    y0, y1, fy = linear_taps(H, sh)
    a1, a0 = fx[None, :, None], fl(F32(1) - fx)[None, :, None]
    b1, b0 = fy[:, None, None], fl(F32(1) - fy)[:, None, None]
    h = fl(fl(S[:, x0] * a0) + fl(S[:, x1] * a1))
    return fl(fl(h[y0] * b0) + fl(h[y1] * b1))


def linear_f64(img, sh, sw):
    """The same formulas with the arithmetic in float64; fx / fy are still cast to float32 first, as the rules say."""
    S = np.asarray(img, dtype=np.float64)
    H, W = S.shape[:2]
    x0, x1, fx = linear_taps(W, sw)
    y0, y1, fy = linear_taps(H, sh)
    fx, fy = fx.astype(np.float64), fy.astype(np.float64)
    a1, a0 = fx[None, :, None], (1.0 - fx)[None, :, None]
    b1, b0 = fy[:, None, None], (1.0 - fy)[:, None, None]
    h = S[:, x0] * a0 + S[:, x1] * a1
    return h[y0] * b0 + h[y1] * b1


def nearest(mask, sh, sw):
    """mask [H, W] -> [sh, sw], same dtype."""
    H, W = mask.shape
    return mask[nearest_index(H, sh)][:, nearest_index(W, sw)]


def bbox(mask):
    """extract_bboxes (img_utils.py:379-394) of one mask: (y1, x1, y2, x2), ends exclusive, four zeros when no byte is valid
    (valid = neither 0 nor 255, :400)."""
    m = (mask != 0) & (mask != 255)
    rows, cols = np.where(m.any(axis=1))[0], np.where(m.any(axis=0))[0]
    if rows.size == 0:
        return 0, 0, 0, 0
    return int(rows[0]), int(cols[0]), int(rows[-1]) + 1, int(cols[-1]) + 1


def scaled_object(obj, scale):
    """The host callback of datapath.draw_sample_params built on this restatement: obj = (image uint8 [H,W,3], mask uint8 [H,W])."""
    img, mask = obj
    sh, sw = scaled_size(mask.shape[0], mask.shape[1], scale)
    return linear(img, sh, sw), nearest(mask, sh, sw)


class StubBank:
    """What draw_sample_params needs of a bank, on the host: __len__ and bbox from the restatement."""

    def __init__(self, objects):
        self.objects = objects

    def __len__(self):
        return len(self.objects)

    def bbox(self, index, scale):
        mask = self.objects[index][1]
        return bbox(nearest(mask, *scaled_size(mask.shape[0], mask.shape[1], scale)))
