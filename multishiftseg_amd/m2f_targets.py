"""The targets of a Mask2Former train step, built from the label maps where they already are: on the device.

The reference builds them per image on the host -- `prepare_input` (train_m2f.py:342-385): `target[b].cpu().numpy()`, np.unique,
one `sem_seg == class_id` map per class and the OOD map -- and `prepare_targets` (lib/network/mask2former/maskformer_model.py:
316-339) pads every mask stack to the batch's size rounded up to SIZE_DIVISIBILITY. `prepare_targets` here is both in one call on
the kernels of csrc/m2f_targets.hip: two launches find the classes of every image, one launch writes the padded masks and OOD
maps in the packed layout the matcher and the criterion read (HungarianMatcher._pack_targets), so they are never concatenated or
copied again. One small copy reaches the host: tstart, B + 1 int32, because `counts` and max T_b size the criterion's tensors.
There is no CPU path.

Deviation from the reference, deliberate: a negative label value is neither a class nor OOD. The reference keeps it as a class
(`classes < label_threshold` holds for it) with a negative label, which its own criterion then indexes out of range.
A value equal to label_threshold is neither a class nor OOD, and ignore_label is never OOD: both as in the reference, whose two
comparisons are strict.
"""
import torch

from . import kernels as K


class M2FTargets(list):
    """The per-image target dicts of the reference -- "labels" int64 [T_b], "masks" bool [T_b,Hp,Wp], "ood_mask" bool [Hp,Wp],
    "sem_seg" [H,W], all on the device -- as views of the packed buffers in `packed` = (tmask uint8 [sum T,Hp,Wp], tstart int32
    [B+1], labels int32 [sum T], counts): what HungarianMatcher._pack_targets returns, and hands back as it is for this class."""

    def __init__(self, dicts, packed, ood):
        super().__init__(dicts)
        self.packed = packed
        self.ood = ood              # uint8 [B,Hp,Wp]: what the "ood_mask" entries are views of


def padded_size(H, W, size_divisibility):
    """(Hp, Wp): H and W rounded up to size_divisibility (ImageList.from_tensors); 0 or 1 = no padding."""
    d = int(size_divisibility)
    if d < 0:
        raise ValueError(f"size_divisibility {size_divisibility} is negative")
    if d <= 1:
        return int(H), int(W)
    return (int(H) + d - 1) // d * d, (int(W) + d - 1) // d * d


def prepare_targets(sem_seg, size_divisibility=32, ignore_label=255, label_threshold=100):
    """prepare_input (train_m2f.py:342-385) and prepare_targets (maskformer_model.py:316-339) for a batch of label maps sem_seg
    [B,H,W] (or one map [H,W]), int64 / int32 / uint8 on the device -> M2FTargets. A class is a value in [0, label_threshold)
    (label_threshold <= 128), in ascending order per image; OOD is `> label_threshold` and not ignore_label."""
    if not isinstance(sem_seg, torch.Tensor) or not sem_seg.is_cuda:
        raise RuntimeError("prepare_targets runs on an MI355X only (a CUDA label map); there is no CPU path")
    if sem_seg.dim() == 2:
        sem_seg = sem_seg[None]
    if sem_seg.dim() != 3:
        raise ValueError(f"prepare_targets takes label maps [B,H,W] or [H,W], got {tuple(sem_seg.shape)}")
    sem = sem_seg.contiguous()
    B, H, W = sem.shape
    Hp, Wp = padded_size(H, W, size_divisibility)
    tstart, labels_buf, rank, _ = K.m2f_targets_count(sem, label_threshold)
    host = torch.zeros(B + 1, dtype=torch.int32).pin_memory()
    host.copy_(tstart, non_blocking=True)                   # the one copy to the host
    torch.cuda.current_stream(sem.device).synchronize()
    starts = host.tolist()
    counts = [starts[b + 1] - starts[b] for b in range(B)]
    total_t = starts[B]
    tmask, ood = K.m2f_targets_fill(sem, tstart, rank, total_t, (Hp, Wp), label_threshold, ignore_label)
    labels = labels_buf[:total_t]
    labels64, masks, oods = labels.to(torch.int64), tmask.view(torch.bool), ood.view(torch.bool)
    dicts = [{"labels": labels64[starts[b]:starts[b + 1]], "masks": masks[starts[b]:starts[b + 1]], "ood_mask": oods[b], "sem_seg": sem_seg[b]}
             for b in range(B)]
    return M2FTargets(dicts, (tmask, tstart, labels, counts), ood)
