#!/usr/bin/env python3
"""SegMeter.update (csrc/metric.hip, mss_seg_hist) against the stock-torch composition it replaces, in one process on one device:

    fused   SegMeter.update(logits [B,19,H,W] f32, labels int64)      84 B/px (19 x 4 logits + 8 label)
    u8map   SegMeter.update(prediction map uint8, labels int64)        9 B/px
    torch   pred = logits.argmax(1); k = (gt >= 0) & (gt < n); hist += bincount(n * gt[k] + pred[k], minlength=n*n)

at 1 x 19 x 1024 x 2048 and 2 x 19 x 700 x 700. The three are timed in alternation, WINDOWS windows of ITERS calls each between two
device events (the window ends in a synchronise), after a warm-up of every shape; each row gives the median window and the spread.
TB/s is algorithmic bytes over that time, to be set against the read-only stream calibration (profiles/r06/measured_peaks.json).
Labels are block-uniform (a label map's large regions) and the logits agree with them on ~80 % of the pixels. One JSON line per row.
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from multishiftseg_amd.metric import SegMeter  # noqa: E402

N_CL, WINDOWS, ITERS = 19, 7, 100


def inputs(B, H, W, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    coarse = torch.randint(0, N_CL, (B, (H + 31) // 32, (W + 31) // 32), generator=g, device="cuda")
    label = coarse.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :H, :W].contiguous()
    label[torch.rand((B, H, W), generator=g, device="cuda") < 0.05] = 255
    logits = torch.randn((B, N_CL, H, W), generator=g, device="cuda")
    agree = torch.rand((B, H, W), generator=g, device="cuda") < 0.8
    logits.scatter_add_(1, label.clamp(max=N_CL - 1).unsqueeze(1), 4.0 * agree.unsqueeze(1).float())
    return logits, label


def window(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(ITERS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / ITERS


def main():
    if not torch.cuda.is_available():
        raise SystemExit("bench_seg_metric: needs the GPU (a CPU run measures nothing)")
    for B, H, W in ((1, 1024, 2048), (2, 700, 700)):
        logits, label = inputs(B, H, W, 7)
        pred8 = logits.argmax(1).to(torch.uint8)
        fused, u8map = SegMeter(N_CL), SegMeter(N_CL)
        thist = torch.zeros(N_CL * N_CL, dtype=torch.int64, device="cuda")

        def stock():
            pred = logits.argmax(1)
            k = (label >= 0) & (label < N_CL)
            thist.add_(torch.bincount(N_CL * label[k] + pred[k], minlength=N_CL * N_CL))
        runs = {"fused": lambda: fused.update(logits, label), "u8map": lambda: u8map.update(pred8, label), "torch": stock}
        for fn in runs.values():                       # every shape once before any window; and the three must agree
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        assert torch.equal(torch.from_numpy(fused.hist()).reshape(-1), thist.cpu()) and (fused.hist() == u8map.hist()).all()
        times = {k: [] for k in runs}
        for _ in range(WINDOWS):
            for k, fn in runs.items():
                times[k].append(window(fn))
        px = B * H * W
        base = statistics.median(times["torch"])
        for k, nbytes in (("fused", 84.0), ("u8map", 9.0), ("torch", 84.0)):
            ms = statistics.median(times[k])
            print(json.dumps(dict(route=k, shape=[B, N_CL, H, W], ms=round(ms, 4), ms_min=round(min(times[k]), 4), ms_max=round(max(times[k]), 4),
                                  alg_bytes_per_px=nbytes, TBs=round(px * nbytes / ms / 1e9, 3), speedup_vs_torch=round(base / ms, 2))), flush=True)


if __name__ == "__main__":
    main()
