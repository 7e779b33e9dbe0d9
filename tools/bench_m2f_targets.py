"""The targets of one Mask2Former train step: prepare_targets (multishiftseg_amd/m2f_targets.py: three launches and one copy of
B + 1 integers) against the reference formulation restated in numpy / torch in the same process, on the same device and the same
synthetic label maps (synth.synth_targets, which start on the device as datapath.make_pair_batch leaves them):

  (a) per image `.cpu().numpy()`, np.unique, one comparison per class and the OOD map (train_m2f.py:342-385), the zero padding to
      the size divisibility (maskformer_model.py:316-339), `.to(device)`, then HungarianMatcher._pack_targets;
  (b) prepare_targets, then the same _pack_targets call (which hands the pack back).

    python tools/bench_m2f_targets.py [--out profiles/m2f_targets/bench.json] [--rounds 10]

Shapes: 16 x 704 x 704 and 2 x 1024 x 2048, int64 labels, divisibility 32. The two sides alternate (3 warm-up rounds, then `rounds`
timed ones, median per side, wall clock around a call that ends synchronised). The fill launch is also timed alone with device
events into buffers of the caller's; its bytes (every byte of tmask and ood written, every label read) over that time is held
against the write-only calibration of mss_peak_stream_f32 (4.85 TB/s, profiles/r06/measured_peaks.json). Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WRITE_ONLY_TBS = 4.85           # profiles/r06/measured_peaks.json: mss_peak_stream_f32, the write-only variant
SHAPES = [(16, 704, 704), (2, 1024, 2048)]


def host_formulation(sem, size_divisibility=32, ignore_label=255, label_threshold=100):
    """train_m2f.py:342-385 and maskformer_model.py:316-339, one image at a time, from the device and back to it."""
    B, H, W = sem.shape
    d = size_divisibility
    Hp, Wp = ((H + d - 1) // d * d, (W + d - 1) // d * d) if d > 1 else (H, W)
    targets = []
    for b in range(B):
        sem_seg_gt = sem[b].cpu().numpy()
        classes = np.unique(sem_seg_gt)
        classes = classes[classes < label_threshold]
        masks = [sem_seg_gt == class_id for class_id in classes]
        ood = (sem_seg_gt > label_threshold) & (sem_seg_gt != ignore_label)
        if len(masks) == 0:
            gt_masks = torch.zeros((0, H, W), dtype=torch.bool)
        else:
            gt_masks = torch.stack([torch.from_numpy(np.ascontiguousarray(x.copy())) for x in masks])
        ood = torch.from_numpy(np.ascontiguousarray(ood.copy()))
        padded = torch.zeros((gt_masks.shape[0], Hp, Wp), dtype=gt_masks.dtype)
        padded[:, :H, :W] = gt_masks
        padded_ood = torch.zeros((Hp, Wp), dtype=gt_masks.dtype)
        padded_ood[:H, :W] = ood
        targets.append({"labels": torch.tensor(classes, dtype=torch.int64).to(sem.device), "masks": padded.to(sem.device),
                        "ood_mask": padded_ood.to(sem.device), "sem_seg": sem[b]})
    return targets


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def device_ms(fn, rounds):
    ts = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts)


def measure(shape, rounds):
    from multishiftseg_amd import HungarianMatcher, prepare_targets, synth
    from multishiftseg_amd import kernels as K
    B, H, W = shape
    sem = torch.from_numpy(synth.synth_targets(0, B // 2, H, W)).cuda()
    m = HungarianMatcher()

    def host():
        return m._pack_targets(host_formulation(sem), "cuda")

    def hip():
        return m._pack_targets(prepare_targets(sem), "cuda")
    a, b = host(), hip()
    same = all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    for _ in range(3):
        hip()
        host()
    th, tr = [], []
    for _ in range(rounds):
        th.append(wall(hip))
        tr.append(wall(host))
    tmask, tstart, labels, counts = b
    total_t, (Hp, Wp) = tmask.shape[0], tmask.shape[1:]
    _, _, rank, _ = K.m2f_targets_count(sem)
    ood = torch.zeros((B, Hp, Wp), device="cuda", dtype=torch.uint8)
    fill_ms = device_ms(lambda: K.m2f_targets_fill(sem, tstart, rank, total_t, (Hp, Wp), tmask=tmask, ood=ood), max(rounds, 20))
    count_ms = device_ms(lambda: K.m2f_targets_count(sem), max(rounds, 20))
    fill_bytes = total_t * Hp * Wp + B * Hp * Wp + sem.numel() * sem.element_size()
    tbs = fill_bytes / (fill_ms * 1e-3) / 1e12
    return {"shape": list(shape), "padded": [Hp, Wp], "targets_per_image": counts, "same_pack_as_host_formulation": same,
            "host_formulation_ms": statistics.median(tr), "host_formulation_ms_min_max": [min(tr), max(tr)],
            "prepare_targets_ms": statistics.median(th), "prepare_targets_ms_min_max": [min(th), max(th)],
            "ratio": statistics.median(tr) / statistics.median(th),
            "device_ms": {"fill_launch": fill_ms, "count_launches": count_ms},
            "fill_bytes": {"written": total_t * Hp * Wp + B * Hp * Wp, "read": sem.numel() * sem.element_size(), "total": fill_bytes},
            "fill_TB_per_s": tbs, "fill_fraction_of_write_only_calibration": tbs / WRITE_ONLY_TBS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_m2f_targets needs an MI355X: there is no CPU measurement path")
    res = {"device": torch.cuda.get_device_name(0), "write_only_calibration_TB_per_s": WRITE_ONLY_TBS, "rounds": args.rounds,
           "shapes": [measure(s, args.rounds) for s in SHAPES]}
    res["prepare_targets_faster_at_every_shape"] = all(s["prepare_targets_ms"] < s["host_formulation_ms"] for s in res["shapes"])
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
