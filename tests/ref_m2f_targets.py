"""Plain numpy restatement of the reference's host-side target build, for the tests of multishiftseg_amd/m2f_targets.py:

  * prepare_input, train_m2f.py:342-385: per image `classes = np.unique(sem_seg)`, `classes = classes[classes < label_threshold]`,
    `masks = [sem_seg == class_id for class_id in classes]`, `ood = (sem_seg > label_threshold) & (sem_seg != ignore_label)`;
  * prepare_targets, lib/network/mask2former/maskformer_model.py:316-339: zeros of the padded size, the masks (and the OOD map)
    copied into the top left corner.

Written from the reference's text, statement by statement. `drop_negative` is the one documented deviation of the product (a
negative value is no class); with drop_negative=False this is the reference as it stands.
"""
import numpy as np


def padded_size(H, W, size_divisibility):
    """ImageList.from_tensors: the batch's size rounded up to size_divisibility (0 or 1: as it is)."""
    d = int(size_divisibility)
    if d > 1:
        return (H + d - 1) // d * d, (W + d - 1) // d * d
    return H, W


def prepare_targets(sem, size_divisibility=32, ignore_label=255, label_threshold=100, drop_negative=True):
    """sem [B,H,W] integer array -> list over images of {"labels" int64 [T], "masks" bool [T,Hp,Wp], "ood_mask" bool [Hp,Wp]}."""
    sem = np.asarray(sem)
    B, H, W = sem.shape
    Hp, Wp = padded_size(H, W, size_divisibility)
    out = []
    for b in range(B):
        sem_seg_gt = sem[b]
        classes = np.unique(sem_seg_gt)                                     # ascending
        classes = classes[classes < label_threshold]
        if drop_negative:
            classes = classes[classes >= 0]
        masks = [sem_seg_gt == class_id for class_id in classes]
        ood = (sem_seg_gt > label_threshold) & (sem_seg_gt != ignore_label)
        padded = np.zeros((len(masks), Hp, Wp), dtype=bool)
        for i, m in enumerate(masks):
            padded[i, :H, :W] = m
        padded_ood = np.zeros((Hp, Wp), dtype=bool)
        padded_ood[:H, :W] = ood
        out.append({"labels": classes.astype(np.int64), "masks": padded, "ood_mask": padded_ood})
    return out
