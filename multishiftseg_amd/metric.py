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
    """update(anomaly_score, target) per batch, compute() at the end of the sweep.

    The state is a multiset of 32-bit order-preserving keys per class, and compute() sorts before it measures: the union of two
    meters' keys therefore measures exactly what one meter fed both meters' maps does, whatever the order. merge() forms that
    union in one process, all_gather() over the ranks of a process group; keys() / extend_keys() are the dense form
    in which keys leave and enter a meter.

    Scores are finite or infinite float32 (denormals keep their place, -0.0 and 0.0 are one score). NaN scores are outside the
    contract: the reference raises on them, and here they would silently sort above +inf or below -inf by their sign bit.
    `recall_level` is the recall at which the FPR is read (the reference's 0.95); any level in [0, 1] is honoured, recall 0
    included when inliers score above every OOD pixel."""

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
        self._dense = []           # (id_in keys, id_out keys): dense int32 arrays taken in whole (extend_keys, all_gather)
        self._gathered = False     # all_gather() ran: a second one would count the peers twice
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

    def _device(self):
        """Where the keys live, None for a meter that holds none."""
        if self._chunks:
            return self._chunks[0][0].device
        return self._dense[0][0].device if self._dense else None

    def _totals(self):
        """(#id_in, #id_out) of every lane chunk -- one D2H copy per counter pool -- and of the whole meter, dense chunks included."""
        pools = {}
        for _, _, _, pool, _ in self._chunks:
            pools.setdefault(id(pool), pool)
        host = {k: p.tolist() for k, p in pools.items()}                          # the sweep's only D2H before the result
        totals = []
        for _, _, _, pool, row in self._chunks:
            lanes = host[id(pool)][row]
            totals.append((sum(v & 0xFFFFFFFF for v in lanes), sum((v & 0xFFFFFFFFFFFFFFFF) >> 32 for v in lanes)))
        N = sum(t[0] for t in totals) + sum(n.numel() for n, _ in self._dense)
        P = sum(t[1] for t in totals) + sum(p.numel() for _, p in self._dense)
        return totals, N, P

    def _gather(self, totals, neg_out, pos_out):
        """Every chunk's keys -> its slice of the caller's two arrays (at least one element each, N and P of _totals used): a map's
        lane segments with one kernel, a dense chunk with one copy. Every used element is written."""
        np_, pp_, no, po = neg_out.data_ptr(), pos_out.data_ptr(), 0, 0
        for (keys, first, cap, pool, row), (a, b) in zip(self._chunks, totals):   # every map's lane segments -> its slice of the two arrays
            call("mss_oodm_gather_lanes_u32", ctypes.c_void_p(keys.data_ptr() + 4 * first), cap, ctypes.c_void_p(pool.data_ptr() + 8 * self._LANES * row),
                 ctypes.c_void_p(np_ + 4 * no), ctypes.c_void_p(pp_ + 4 * po))
            no, po = no + a, po + b
        for neg, pos in self._dense:
            neg_out[no:no + neg.numel()].copy_(neg)
            pos_out[po:po + pos.numel()].copy_(pos)
            no, po = no + neg.numel(), po + pos.numel()

    def compute(self):
        """(auroc, aupr, fpr) as Python floats, or None if there is no in- or no out-of-distribution pixel."""
        if not self._chunks and not self._dense:
            return None
        totals, N, P = self._totals()
        if not N or not P:
            return None
        dev = self._device()
        neg_in, pos_in = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(P, dtype=torch.int32, device=dev)
        self._gather(totals, neg_in, pos_in)
        pos, neg = self._sorted(pos_in), self._sorted(neg_in)
        P, N = pos.numel(), neg.numel()
        nb = _lib.value("mss_oodm_rank_blocks", P)
        u2 = torch.empty(nb, dtype=torch.int64, device=pos.device)
        ap = torch.empty(nb, dtype=torch.float64, device=pos.device)
        out = torch.empty(3, dtype=torch.float64, device=pos.device)
        call("mss_oodm_measures_f64", ptr(pos), P, ptr(neg), N, ctypes.c_double(self.recall_level), ptr(u2), ptr(ap), ptr(out))
        auroc, aupr, fpr = out.tolist()
        return auroc, aupr, fpr

    # ---- combining meters ------------------------------------------------------------------------------------------------------
    def keys(self):
        """(id_in keys, id_out keys) seen so far: two dense, unsorted int32 device tensors -- the gather step of compute(). Two empty
        tensors for an empty meter."""
        totals, N, P = self._totals()
        dev = self._device()
        if dev is None:
            dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        # one spare element: the gather kernel is handed a valid address for a class without a pixel too (it writes nothing there)
        neg, pos = torch.zeros(N + 1, dtype=torch.int32, device=dev), torch.zeros(P + 1, dtype=torch.int32, device=dev)
        self._gather(totals, neg, pos)
        return neg[:N], pos[:P]

    def extend_keys(self, neg, pos):
        """Take dense key arrays (what keys() returns) in as if their pixels had been streamed. The tensors are kept by reference
        and never written."""
        for t in (neg, pos):
            if t.dtype != torch.int32 or t.dim() != 1:
                raise ValueError(f"OODMeter.extend_keys: keys are one-dimensional int32 tensors, got {t.dtype} {tuple(t.shape)}")
        if neg.numel() or pos.numel():
            if not (neg.is_cuda and pos.is_cuda):
                raise RuntimeError("OOD metrics (multishiftseg_amd) run on an MI355X only; there is no CPU path")
            dev = self._device()
            if neg.device != pos.device or (dev is not None and dev != neg.device):
                raise ValueError(f"OODMeter.extend_keys: keys on {neg.device} / {pos.device}, the meter's on {dev}")
            self._dense.append((neg.detach().contiguous(), pos.detach().contiguous()))
        return self

    def merge(self, other):
        """Afterwards this meter measures the union of both meters' pixels; `other` stays valid and unchanged (its key buffers are
        shared by reference: nothing writes them after the update that filled them)."""
        if (other.id_in, other.id_out, other.recall_level) != (self.id_in, self.id_out, self.recall_level):
            raise ValueError(f"OODMeter.merge: (train_id_in, train_id_out, recall_level) = {(other.id_in, other.id_out, other.recall_level)} "
                             f"into {(self.id_in, self.id_out, self.recall_level)}")
        a, b = self._device(), other._device()
        if a is not None and b is not None and a != b:
            raise ValueError(f"OODMeter.merge: keys on {b} into keys on {a}")
        self._chunks += other._chunks
        self._dense += other._dense
        return self

    def all_gather(self, group=None):
        """A collective: afterwards every rank's meter holds the keys of all ranks of `group`, so compute() returns on every rank
        what one meter fed every rank's maps returns (the same tuple, or None). Without an initialised group, or with one rank,
        nothing happens (ddp.is_active: MSS_DDP_FORCE=1 runs the collectives in a one-rank group too). Two collectives: the 2 x
        world key counts, then the keys padded to the largest count of each class -- device to device where the group's backend
        is nccl (RCCL), staged through host tensors over ddp.host_group(group) otherwise. The padding is sliced off here: no
        padding element is ever read. A second call before reset() raises: it would count the peers twice."""
        from . import ddp
        import torch.distributed as dist
        if self._gathered:
            raise RuntimeError("OODMeter.all_gather: the peers' keys are already here; reset() before the next sweep")
        if not (dist.is_available() and ddp.is_active(group)):
            return self
        world = dist.get_world_size(group)
        neg, pos = self.keys()
        on_device = "nccl" in str(dist.get_backend(group))
        dev = neg.device if neg.is_cuda else torch.device("cuda", torch.cuda.current_device())
        if on_device:
            where, g = dev, group
        else:
            where, g = torch.device("cpu"), ddp.host_group(group)
        counts = torch.zeros(2 * world, dtype=torch.int64, device=where)
        dist.all_gather_into_tensor(counts, torch.tensor([neg.numel(), pos.numel()], dtype=torch.int64, device=where), group=g)
        counts = counts.tolist()
        ns, ps = counts[0::2], counts[1::2]
        mn, mp = max(ns), max(ps)
        self._chunks, self._dense, self._gathered = [], [], True
        if mn + mp == 0:                                     # every rank knows: no rank enters the key exchange
            return self
        send = torch.zeros(mn + mp, dtype=torch.int32, device=where)          # [id_in keys, padding | id_out keys, padding]
        send[:neg.numel()].copy_(neg)
        send[mn:mn + pos.numel()].copy_(pos)
        recv = torch.zeros(world * (mn + mp), dtype=torch.int32, device=where)
        dist.all_gather_into_tensor(recv, send, group=g)
        recv = recv.to(dev)
        for r in range(world):
            at = r * (mn + mp)
            if ns[r] or ps[r]:
                self._dense.append((recv[at:at + ns[r]], recv[at + mn:at + mn + ps[r]]))
        return self


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
