"""Pixel-level OOD metrics on the GPU: host-side mirror of ``lib/utils/metric.py``'s
``eval_ood_measure`` (:170-180) with the same arguments and return convention -- ``(auroc, aupr, fpr)`` or ``None``
when one of the two classes has no pixel -- over device tensors, so the evaluation sweep (test_deeplab.py:84-102,
train_deeplab.py:223-241) never copies a score map to the host. ``OODMeter`` is the streaming form of the
reference's "append every batch, concatenate, evaluate" loop.

All arithmetic is in libmss_hip.so (csrc/metric.hip): exact rank statistics on sorted 32-bit keys, no binning.

The segmentation half of the same file (metric.py:10-64) is here too: ``SegMeter`` accumulates the confusion matrix of the
closed-set prediction on the device (mss_seg_hist: the argmax over the logits is fused, one launch per batch, no host
synchronisation) and ``hist_info`` / ``compute_metric`` / ``compute_score`` / ``compute_score_per_class`` keep the reference's names,
arguments and return conventions. The three scorers are host arithmetic on numpy arrays and need no GPU.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import call, ptr


def _flat(score, label):
    if not (score.is_cuda and label.is_cuda):
        raise RuntimeError("OOD metrics (multishiftseg_amd) run on an MI355X only; there is no CPU path")
    if score.numel() != label.numel():
        raise ValueError(f"score has {score.numel()} elements, label has {label.numel()}")
    # the usual case -- a contiguous float32 score map and int64 labels -- passes through untouched: an update is ONE kernel of a
    # few microseconds, so every tensor method call on the way to it shows (r04: 27 -> see DESIGN 7 per 1024 x 2048 image)
    if score.dtype != torch.float32 or not score.is_contiguous() or score.requires_grad:
        score = score.detach().float().contiguous()
    if label.dtype != torch.int64 or not label.is_contiguous():
        label = label.detach().long().contiguous()
    return score, label


class OODMeter:
    """update(anomaly_score, target) per batch, compute() at the end of the sweep."""

    def __init__(self, train_id_in=0, train_id_out=1, recall_level=0.95):
        if train_id_in == train_id_out:
            raise ValueError("train_id_in and train_id_out must differ")
        self.id_in, self.id_out, self.recall_level = int(train_id_in), int(train_id_out), float(recall_level)
        self.reset()

    _POOL = 256                    # counter rows zeroed per fill kernel
    _LANES = 8                     # counters per update (csrc/metric.hip, mss_oodm_compact_lanes_f32)
    _CHUNK = 4096                  # pixels a workgroup compacts at a time

    def reset(self):
        self._chunks = []          # (key buffer, first slot, cap, pool, row): 8 cap u32 slots from `first slot`, per lane inliers at the front, OOD at the back of its segment
        self._pool, self._pool_ptr, self._used = None, 0, 0

    def _counters(self, device):
        """Index of a zeroed row of 8 packed counters (#id_in | #id_out << 32): one fill kernel per _POOL updates, no tensor view per update."""
        if self._pool is None or self._used == self._POOL or self._pool.device != device:
            self._pool = torch.zeros((self._POOL, self._LANES), dtype=torch.int64, device=device)
            self._pool_ptr, self._used = self._pool.data_ptr(), 0
        self._used += 1
        return self._used - 1

    def update(self, score, label):
        """One kernel per batch, no host synchronisation (the reference copies both maps to the host here)."""
        score, label = _flat(score, label)
        n = score.numel()
        if n == 0:
            return
        if n >= 1 << 32:
            raise ValueError("OODMeter.update: at most 2^32 - 1 pixels per call")
        cap = -(-(-(-n // self._CHUNK)) // self._LANES) * self._CHUNK            # = mss_oodm_compact_lanes_cap(n)
        keys = torch.empty(self._LANES * cap, dtype=torch.int32, device=score.device)
        row = self._counters(score.device)
        call("mss_oodm_compact_lanes_f32", ptr(score), ptr(label), n, self.id_in, self.id_out, ptr(keys),
             ctypes.c_void_p(self._pool_ptr + 8 * self._LANES * row))
        self._chunks.append((keys, 0, cap, self._pool, row))

    def update_many(self, pairs):
        """The same for a sweep that already holds its maps: `pairs` = iterable of (anomaly_score, target) batches, handed to the device
        sixteen per launch (mss_oodm_compact_lanes_batch_f32) -- one kernel launch, one key buffer and one Python round trip per 16 maps
        instead of per map (an update is ~8 us of kernel behind ~20 us of host work). Same result as update() in a loop."""
        group = []
        for score, label in pairs:
            score, label = _flat(score, label)
            n = score.numel()
            if n >= 1 << 32:
                raise ValueError("OODMeter.update_many: at most 2^32 - 1 pixels per map")
            if n:
                group.append((score, label, n))
            if len(group) == _lib.MSS_OODM_BATCH:
                self._flush(group)
                group = []
        if group:
            self._flush(group)

    def _flush(self, group):
        dev = group[0][0].device
        if any(s.device != dev for s, _, _ in group):
            raise ValueError("OODMeter.update_many: all maps of a sweep must live on one device")
        caps = [-(-(-(-n // self._CHUNK)) // self._LANES) * self._CHUNK for _, _, n in group]
        keys = torch.empty(self._LANES * sum(caps), dtype=torch.int32, device=dev)       # one buffer, a segment of 8 cap per map
        b = _lib.MssOodmBatch()
        kp, off = keys.data_ptr(), 0
        for m, ((score, label, n), cap) in enumerate(zip(group, caps)):
            row = self._counters(dev)
            b.score[m], b.label[m], b.n[m] = score.data_ptr(), label.data_ptr(), n
            b.keys[m], b.lane_counts[m] = kp + 4 * off, self._pool_ptr + 8 * self._LANES * row
            self._chunks.append((keys, off, cap, self._pool, row))
            off += self._LANES * cap
        call("mss_oodm_compact_lanes_batch_f32", ctypes.byref(b), len(group), self.id_in, self.id_out)

    @staticmethod
    def _sorted(keys):
        n = keys.numel()
        out = torch.empty_like(keys)
        temp = torch.empty(_lib.value("mss_oodm_sort_temp_bytes", n), dtype=torch.uint8, device=keys.device)
        call("mss_oodm_sort_u32", ptr(keys), ptr(out), n, ptr(temp), temp.numel())
        return out

    def compute(self):
        """(auroc, aupr, fpr) as Python floats, or None if there is no in- or no out-of-distribution pixel."""
        if not self._chunks:
            return None
        pools = {}
        for _, _, _, pool, _ in self._chunks:
            pools.setdefault(id(pool), pool)
        host = {k: p.tolist() for k, p in pools.items()}                          # the sweep's only D2H before the result
        totals = []
        for _, _, _, pool, row in self._chunks:
            lanes = host[id(pool)][row]
            totals.append((sum(v & 0xFFFFFFFF for v in lanes), sum((v & 0xFFFFFFFFFFFFFFFF) >> 32 for v in lanes)))
        N, P = sum(t[0] for t in totals), sum(t[1] for t in totals)
        if not N or not P:
            return None
        dev = self._chunks[0][0].device
        neg_in, pos_in = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.int32, device=dev)
        np_, pp_, no, po = neg_in.data_ptr(), pos_in.data_ptr(), 0, 0
        for (keys, first, cap, pool, row), (a, b) in zip(self._chunks, totals):   # every map's lane segments -> its slice of the two arrays
            call("mss_oodm_gather_lanes_u32", ctypes.c_void_p(keys.data_ptr() + 4 * first), cap, ctypes.c_void_p(pool.data_ptr() + 8 * self._LANES * row),
                 ctypes.c_void_p(np_ + 4 * no), ctypes.c_void_p(pp_ + 4 * po))
            no, po = no + a, po + b
        pos, neg = self._sorted(pos_in), self._sorted(neg_in)
        P, N = pos.numel(), neg.numel()
        nb = _lib.value("mss_oodm_rank_blocks", P)
        u2 = torch.empty(nb, dtype=torch.int64, device=pos.device)
        ap = torch.empty(nb, dtype=torch.float64, device=pos.device)
        out = torch.empty(3, dtype=torch.float64, device=pos.device)
        call("mss_oodm_measures_f64", ptr(pos), P, ptr(neg), N, ctypes.c_double(self.recall_level), ptr(u2), ptr(ap), ptr(out))
        auroc, aupr, fpr = out.tolist()
        return auroc, aupr, fpr


def eval_ood_measure(conf, seg_label, train_id_in=0, train_id_out=1):
    """Drop-in for lib/utils/metric.py:170-180 on CUDA tensors (any shape, equal element counts)."""
    m = OODMeter(train_id_in, train_id_out)
    m.update(conf, seg_label)
    return m.compute()


# ---- closed-set segmentation metrics (lib/utils/metric.py:10-64) --------------------------------------------------------------
_SEG_F32, _SEG_U8, _SEG_I64 = 0, 1, 8                # mss_seg_hist's pred_kind


class SegMeter:
    """update(pred, target) per batch, compute() at the end of the sweep: the streaming form of the reference's "hist_info per
    image, compute_metric over the list" loop. The table is int64 [n_cl * n_cl + 1]: the confusion matrix (row = label, column =
    prediction) and one last counter for labelled pixels whose map prediction lies outside 0 .. n_cl-1."""

    _CHUNK = 4096                  # pixels of one image a workgroup counts (csrc/metric.hip, SEG_CHUNK)
    _MAX_CL = 32

    def __init__(self, n_cl=19):
        n_cl = int(n_cl)
        if not 2 <= n_cl <= self._MAX_CL:
            raise ValueError(f"SegMeter: 2 <= n_cl <= {self._MAX_CL}, got {n_cl}")
        self.n_cl = n_cl
        self.reset()

    def reset(self):
        self._table = None

    def _counters(self, device):
        if self._table is None:
            self._table = torch.zeros(self.n_cl * self.n_cl + 1, dtype=torch.int64, device=device)
        elif self._table.device != device:
            raise ValueError(f"SegMeter: the table lives on {self._table.device}, this batch on {device}")
        return self._table

    def update(self, pred, target):
        """pred: float logits [B, n_cl, H, W] (the argmax is fused; a channel slice with unit pixel stride goes in without a copy) or
        an integer prediction map [B, H, W]; target [B, H, W], uint8 or int64 (anything else is converted). One kernel, no host
        synchronisation (the reference copies both maps to the host here)."""
        if not (pred.is_cuda and target.is_cuda):
            raise RuntimeError("segmentation metrics (multishiftseg_amd) run on an MI355X only; there is no CPU path")
        n = self.n_cl
        pred = pred.detach()
        if pred.is_floating_point():
            if pred.dim() != 4 or pred.shape[1] != n:
                raise ValueError(f"SegMeter.update: logits are [B, {n}, H, W], got {tuple(pred.shape)}")
            B, _, H, W = pred.shape
            HW = H * W
            if pred.dtype != torch.float32:
                pred = pred.float()
            sb, sc, sh, sw = pred.stride()
            if HW and B and not (sw == 1 and sh == W and sc >= HW and (B == 1 or sb >= n * sc)):
                pred = pred.contiguous()
                sb, sc = n * HW, HW
            if B == 1:
                sb = n * sc                      # one image: its stride is never applied
            kind = _SEG_F32
        else:
            if pred.dim() != 3:
                raise ValueError(f"SegMeter.update: a prediction map is [B, H, W], got {tuple(pred.shape)}")
            B, H, W = pred.shape
            HW = H * W
            if pred.dtype not in (torch.uint8, torch.int64):
                pred = pred.long()
            if not pred.is_contiguous():
                pred = pred.contiguous()
            sb = sc = 0
            kind = _SEG_U8 if pred.dtype == torch.uint8 else _SEG_I64
        if tuple(target.shape) != (B, H, W):
            raise ValueError(f"SegMeter.update: target {tuple(target.shape)} against a prediction of {(B, H, W)}")
        target = target.detach()
        if target.dtype not in (torch.uint8, torch.int64):
            target = target.long()
        if not target.is_contiguous():
            target = target.contiguous()
        if B * HW == 0:
            return
        if B * HW >= 1 << 32:
            raise ValueError("SegMeter.update: at most 2^32 - 1 pixels per call")
        table = self._counters(pred.device)
        call("mss_seg_hist", ptr(pred), kind, sb, sc, ptr(target), target.element_size(), B, HW, n, ptr(table))

    def _host(self):
        """The whole table on the host, int64 numpy: the sweep's one device-to-host copy."""
        if self._table is None:
            return np.zeros(self.n_cl * self.n_cl + 1, dtype=np.int64)
        return self._table.cpu().numpy()

    def hist(self):
        """int64 [n_cl, n_cl] on the host (numpy), rows = labels, columns = predictions."""
        return self._host()[:-1].reshape(self.n_cl, self.n_cl).copy()

    def compute(self, per_class=False):
        """What compute_metric returns -- (mean_IU, mean_pixel_acc), or (mean_IU, mean_pixel_acc, iu, class_acc) -- or None when no
        pixel was labelled (the reference divides 0 by 0 there). Raises ValueError if a map held predictions outside 0 .. n_cl-1."""
        host = self._host()
        if host[-1]:
            raise ValueError(f"SegMeter: {int(host[-1])} labelled pixels carry a prediction outside 0..{self.n_cl - 1}")
        hist = host[:-1].reshape(self.n_cl, self.n_cl)
        labeled, correct = int(hist.sum()), int(np.trace(hist))
        if labeled == 0:
            return None
        return compute_metric([{"hist": hist, "labeled": labeled, "correct": correct}], per_class)

    @classmethod
    def from_hist(cls, hist):
        """A meter (on the host) that continues from a confusion matrix: int [n_cl, n_cl], numpy or tensor."""
        h = torch.as_tensor(np.asarray(hist.cpu() if isinstance(hist, torch.Tensor) else hist)).to(torch.int64)
        if h.dim() != 2 or h.shape[0] != h.shape[1]:
            raise ValueError(f"SegMeter.from_hist: a square table, got {tuple(h.shape)}")
        m = cls(h.shape[0])
        m._table = torch.zeros(m.n_cl * m.n_cl + 1, dtype=torch.int64)
        m._table[:-1] = h.reshape(-1)
        return m

    def merge(self, other):
        """Add another meter's table (same n_cl) to this one."""
        if other.n_cl != self.n_cl:
            raise ValueError(f"SegMeter.merge: n_cl {other.n_cl} into {self.n_cl}")
        if other._table is not None:
            if self._table is None:
                self._table = other._table.clone()
            else:
                self._table += other._table.to(self._table.device)
        return self

    def all_reduce(self, group=None):
        """Sum the table over the ranks of a process group (integers: exact, in any order). Without an initialised group, or with
        one rank, nothing happens -- ddp.GradAllReduce's convention. A host table (from_hist) travels as it is (gloo)."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) < 2:
            return self
        if self._table is None:
            self._table = torch.zeros(self.n_cl * self.n_cl + 1, dtype=torch.int64,
                                      device="cuda" if dist.get_backend(group) == "nccl" else "cpu")
        dist.all_reduce(self._table, op=dist.ReduceOp.SUM, group=group)
        return self


def hist_info(n_cl, pred, gt):
    """metric.py:10-18 on device tensors: pred is a prediction map shaped like gt (or the logits [B, n_cl, H, W] themselves) ->
    (hist int64 [n_cl, n_cl] numpy, labeled, correct), the two counts as Python ints: the table's sum and trace."""
    m = SegMeter(n_cl)
    if not pred.is_floating_point() and pred.dim() != 3:
        if pred.shape != gt.shape:
            raise ValueError(f"hist_info: pred {tuple(pred.shape)} against gt {tuple(gt.shape)}")
        pred, gt = pred.reshape(1, 1, -1), gt.reshape(1, 1, -1)
    m.update(pred, gt)
    host = m._host()
    if host[-1]:
        raise ValueError(f"hist_info: {int(host[-1])} labelled pixels carry a prediction outside 0..{n_cl - 1}")
    hist = host[:-1].reshape(n_cl, n_cl).copy()
    return hist, int(hist.sum()), int(np.trace(hist))


def compute_metric(results, per_class=False):
    """metric.py:21-39: `results` = dicts with 'hist', 'correct', 'labeled'. The reference's hard-coded 19 is the shape of the
    first hist here."""
    results = list(results)
    hist = np.zeros(np.shape(results[0]["hist"]) if results else (19, 19))
    correct = 0
    labeled = 0
    for d in results:
        hist += d["hist"]
        correct += d["correct"]
        labeled += d["labeled"]
    if per_class:
        iu, mean_IU, class_acc, mean_pixel_acc = compute_score_per_class(hist, correct, labeled)
        return mean_IU, mean_pixel_acc, iu, class_acc
    iu, mean_IU, _, mean_pixel_acc = compute_score(hist, correct, labeled)
    return mean_IU, mean_pixel_acc


def compute_score(hist, correct, labeled):
    """metric.py:42-49: a class that occurs in neither map is 0 / 0 = NaN and drops out of the nanmean."""
    with np.errstate(divide="ignore", invalid="ignore"):
        iu = np.diag(hist) / (hist.sum(1) + hist.sum(0) - np.diag(hist))
        mean_IU = np.nanmean(iu)
        mean_IU_no_back = np.nanmean(iu[1:])
        mean_pixel_acc = np.float64(correct) / np.float64(labeled)
    return iu, mean_IU, mean_IU_no_back, mean_pixel_acc


def compute_score_per_class(hist, correct, labeled):
    """metric.py:51-64: the union is clamped to 1, so an absent class counts as IoU 0 in the mean."""
    intersection = np.diag(hist)
    union = hist.sum(axis=1) + hist.sum(axis=0) - np.diag(hist)
    iu = intersection / np.maximum(union, 1)
    class_acc = intersection / np.maximum(hist.sum(axis=1), 1)
    mean_IU = np.nanmean(iu)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean_pixel_acc = np.float64(correct) / np.float64(labeled)
    return iu, mean_IU, class_acc, mean_pixel_acc
