"""Test helper: an independent numpy restatement of the closed-set segmentation metrics of lib/utils/metric.py:10-64 (hist_info and
the two scorers behind compute_metric), written from their definition rather than copied: the confusion matrix is counted with
np.add.at on (label, prediction) pairs, the scores are the textbook ratios in float64. tests/test_seg_metric_cpu.py holds it to the
reference's own outputs in tests/golden/seg_metrics.npz; the GPU tests then use it at shapes the fixture does not have.

Plain module, imported by the tests that want it; nothing loads it automatically.
"""
import numpy as np


def hist_info(n_cl, pred, gt):
    """-> (hist int64 [n_cl, n_cl] with rows = labels and columns = predictions over the pixels with 0 <= gt < n_cl, labeled, correct)"""
    pred, gt = np.asarray(pred).reshape(-1).astype(np.int64), np.asarray(gt).reshape(-1).astype(np.int64)
    assert pred.shape == gt.shape
    keep = (gt >= 0) & (gt < n_cl)
    hist = np.zeros((n_cl, n_cl), dtype=np.int64)
    np.add.at(hist, (gt[keep], pred[keep]), 1)
    return hist, int(keep.sum()), int((pred[keep] == gt[keep]).sum())


def split_invalid(n_cl, pred, gt):
    """For prediction maps that may hold values outside 0 .. n_cl-1: -> (hist of the labelled pixels with a valid prediction, the
    number of labelled pixels with an invalid one)"""
    pred, gt = np.asarray(pred).reshape(-1).astype(np.int64), np.asarray(gt).reshape(-1).astype(np.int64)
    ok = (pred >= 0) & (pred < n_cl)
    labelled = (gt >= 0) & (gt < n_cl)
    return hist_info(n_cl, pred[ok], gt[ok])[0], int((labelled & ~ok).sum())


def _parts(hist):
    hist = np.asarray(hist, dtype=np.float64)
    inter = np.diag(hist)
    rows, cols = hist.sum(axis=1), hist.sum(axis=0)
    return inter, rows, rows + cols - inter


def score(hist, correct, labeled):
    """compute_score: -> (iu, mean_IU, mean_pixel_acc); a class in neither map is NaN and leaves the mean"""
    inter, _, union = _parts(hist)
    with np.errstate(divide="ignore", invalid="ignore"):
        iu = inter / union
        return iu, np.nanmean(iu), np.float64(correct) / np.float64(labeled)


def score_per_class(hist, correct, labeled):
    """compute_score_per_class: -> (iu, mean_IU, class_acc, mean_pixel_acc); denominators clamped to 1"""
    inter, rows, union = _parts(hist)
    iu = inter / np.maximum(union, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return iu, np.nanmean(iu), inter / np.maximum(rows, 1), np.float64(correct) / np.float64(labeled)


def metric(hist, per_class=False):
    """compute_metric over one table: labeled and correct are its sum and trace"""
    hist = np.asarray(hist)
    labeled, correct = int(hist.sum()), int(np.trace(hist))
    if per_class:
        iu, mean_iu, class_acc, acc = score_per_class(hist, correct, labeled)
        return mean_iu, acc, iu, class_acc
    _, mean_iu, acc = score(hist, correct, labeled)
    return mean_iu, acc


def lattice_logits(rng, B, n_cl, HW):
    """float32 logits in {-1, 0, 1}: every pixel has several maximal classes, so the first-index rule decides"""
    return rng.integers(-1, 2, (B, n_cl, HW)).astype(np.float32)
