"""A device-resident bank of the COCO objects that the anomaly mix pastes.

The reference picks an object per sample, rescales it on the host with cv2.resize (lib/utils/img_utils.py:345-352, INTER_LINEAR
for the image, INTER_NEAREST for the mask) and cuts it to the bounding box of its valid mask pixels (:379-406). Here the decoded
objects are uploaded ONCE as uint8 image and uint8 mask, the bounding box of every (object, scale) pair is computed once on the
device and read back once, and per step one launch (mss_obj_rescale_f32 of libmss_obj.so, include/mss_obj_hip.h) writes the
rescaled and cut objects of the whole batch into the buffers that the paste kernels read. The host keeps the random decisions
(datapath.draw_sample_params) and the small job table; rescale() reads nothing back and copies no pixel.

Resident bytes: 4 * sum(H * W) over the objects (three image bytes and one mask byte per pixel), in ``bank.resident_bytes``; at
most 2^31 - 1 pixels in one bank. A caller shards or rebuilds the bank when its COCO subset does not fit.

The arithmetic is cv2.resize restated (csrc/mss_cv_resize.h, tests/ref_object_bank.py); sizes are int(H * scale), int(W * scale)
in Python float arithmetic. There is no CPU path: a CPU device raises.
"""
import numpy as np
import torch

from . import _lib_obj as L
from ._lib_obj import call, ptr
from .datapath import OOD_SCALES


def scaled_size(H, W, scale):
    """(sh, sw) of img_utils.py:347-348; a size below 1 raises, as cv2.resize does."""
    sh, sw = int(H * scale), int(W * scale)
    if sh < 1 or sw < 1:
        raise ValueError(f"scale {scale} takes a {H} x {W} object to {sh} x {sw}")
    return sh, sw


class ObjectBank:
    """objects: a sequence of (image uint8 [H, W, 3], mask uint8 [H, W]), numpy arrays or tensors. Holds them in two flat device
    buffers (4 * sum(H * W) bytes, ``resident_bytes``) and the [len, len(scales), 4] bounding-box table on the host."""

    def __init__(self, objects, scales=OOD_SCALES, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("multishiftseg_amd.object_bank runs on an MI355X only; there is no CPU path")
        if len(objects) == 0:
            raise ValueError("an object bank needs at least one object")
        imgs, masks, self.shapes, self.offsets = [], [], [], []
        total = 0
        for k, (img, mask) in enumerate(objects):
            img, mask = torch.as_tensor(img), torch.as_tensor(mask)
            if img.dtype != torch.uint8 or mask.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3 \
                    or tuple(mask.shape) != tuple(img.shape[:2]) or img.shape[0] < 1 or img.shape[1] < 1:
                raise TypeError(f"object {k}: expected a uint8 [H, W, 3] image and a uint8 [H, W] mask")
            H, W = int(img.shape[0]), int(img.shape[1])
            self.shapes.append((H, W))
            self.offsets.append(total)
            total += H * W
            imgs.append(img.reshape(-1).cpu())
            masks.append(mask.reshape(-1).cpu())
        if total > L.MSS_OBJ_MAX_PIXELS:
            raise ValueError(f"{total} pixels exceed the {L.MSS_OBJ_MAX_PIXELS} of one bank: shard it")
        self.device = device
        self.pixels = total
        self.resident_bytes = 4 * total
        self.img = torch.cat(imgs).to(device)
        self.mask = torch.cat(masks).to(device)
        self.scales = list(scales)
        self._column = {s: i for i, s in enumerate(self.scales)}
        self._extra = {}                                # (index, scale) -> box, for scales outside the table
        pairs = [(k, s) for k in range(len(self.shapes)) for s in self.scales]
        self.boxes = self._bboxes(pairs).reshape(len(self.shapes), len(self.scales), 4)

    def __len__(self):
        return len(self.shapes)

    def _source(self, index, scale):
        H, W = self.shapes[index]
        return (self.offsets[index], H, W) + scaled_size(H, W, scale)

    def _bboxes(self, pairs):
        """int64 numpy [len(pairs), 4]: one launch per MSS_OBJ_MAX_BBOX_JOBS pairs and one read-back."""
        jobs = torch.tensor([self._source(k, s) for k, s in pairs], dtype=torch.int32).reshape(-1, L.MSS_OBJ_BBOX_JOB_INTS).to(self.device)
        boxes = torch.zeros((len(pairs), 4), device=self.device, dtype=torch.int32)
        with torch.cuda.device(self.device):
            for lo in range(0, len(pairs), L.MSS_OBJ_MAX_BBOX_JOBS):
                n = min(L.MSS_OBJ_MAX_BBOX_JOBS, len(pairs) - lo)
                call("mss_obj_bbox_u8", ptr(self.mask), self.pixels, ptr(jobs[lo:]), n, ptr(boxes[lo:]))
        return boxes.cpu().numpy().astype(np.int64)

    def bbox(self, index, scale):
        """(y1, x1, y2, x2) of the valid pixels of object `index` rescaled by `scale` (extract_bboxes, img_utils.py:379-394), from
        the host table; a scale outside the table costs one launch and is cached."""
        if not 0 <= index < len(self.shapes):
            raise IndexError(f"object {index} of a bank of {len(self.shapes)}")
        col = self._column.get(scale)
        if col is not None:
            return tuple(int(v) for v in self.boxes[index, col])
        key = (index, scale)
        if key not in self._extra:
            self._extra[key] = tuple(int(v) for v in self._bboxes([key])[0])
        return self._extra[key]

    def rescale(self, picks, out=None):
        """picks: [(index, scale), ...] -> (obj_img float32 [B, OHmax, OWmax, 3], values 0..255, obj_mask uint8 [B, OHmax, OWmax]):
        slot b holds, at its origin, the bounding-box window of object `index` rescaled by `scale`; nothing outside the windows is
        written. OHmax / OWmax: the largest window of the batch, at least 1. out=(img, mask): write into the caller's buffers, which
        may be larger. One launch, no read-back."""
        B = len(picks)
        if B < 1:
            raise ValueError("rescale needs at least one pick")
        jobs = []
        for index, scale in picks:
            y1, x1, y2, x2 = self.bbox(index, scale)
            jobs.append(self._source(index, scale) + (y1, x1, y2 - y1, x2 - x1))
        ohm = max(1, max(j[7] for j in jobs))
        owm = max(1, max(j[8] for j in jobs))
        if out is None:
            obj_img = torch.empty((B, ohm, owm, 3), device=self.device, dtype=torch.float32)
            obj_mask = torch.zeros((B, ohm, owm), device=self.device, dtype=torch.uint8)
        else:
            obj_img, obj_mask = out
            if obj_img.device != self.img.device or obj_mask.device != self.img.device:
                raise RuntimeError("the output buffers must live on the bank's device; there is no CPU path")
            if obj_img.dtype != torch.float32 or obj_mask.dtype != torch.uint8 or obj_img.dim() != 4 or obj_img.shape[3] != 3 \
                    or tuple(obj_mask.shape) != tuple(obj_img.shape[:3]) or not obj_img.is_contiguous() or not obj_mask.is_contiguous():
                raise TypeError("out is a contiguous float32 [B, OH, OW, 3] image buffer and a uint8 [B, OH, OW] mask buffer")
            if obj_img.shape[0] != B or obj_img.shape[1] < ohm or obj_img.shape[2] < owm:
                raise ValueError(f"out holds {tuple(obj_img.shape[:3])}, the batch needs at least {(B, ohm, owm)}")
        jobs_t = torch.tensor(jobs, dtype=torch.int32).to(self.device)
        with torch.cuda.device(self.device):
            call("mss_obj_rescale_f32", ptr(self.img), ptr(self.mask), self.pixels, ptr(jobs_t), B, int(obj_img.shape[1]),
                 int(obj_img.shape[2]), ptr(obj_img), ptr(obj_mask))
        return obj_img, obj_mask
