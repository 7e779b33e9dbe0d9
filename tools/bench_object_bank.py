"""The resident object bank (multishiftseg_amd/object_bank.py, csrc/obj_bank.hip) on one MI355X.

    python tools/bench_object_bank.py [--out profiles/object_bank/bench.json] [--rounds 10] [--inner 20] [--loop N]

A bank of 32 objects of 640 x 480 pixels (480 rows) with every mask byte valid, batches of 16 picks: all at scale 1.0, all at 0.5,
and the reference's mix (random.choice over datapath.OOD_SCALES, seeded). Per batch:
  * kernel_ms: the mss_obj_rescale_f32 launch alone, job table already on the device, --inner launches between two device events;
    bytes = 13 per window pixel (12 image + 1 mask) written, over that time, against the write-only stream of
    profiles/r06/measured_peaks.json;
  * rescale_call_ms: bank.rescale as the pipelines call it (job table built and uploaded, buffers allocated), host clock, synchronised;
  * pair_batch_bank_ms / pair_batch_host_ms: the whole datapath.make_pair_batch at 16 x 700 x 700 from 1024 x 2048 maps, once with
    picks and the bank, once -- the call as it was before the bank -- fed host objects that were rescaled beforehand (its zero-filled
    [B, OHmax, OWmax, 3] float32 host array, the copies into it and the upload are inside, the resize itself is not). The two sides
    alternate in one process; their outputs are compared.
--loop N only repeats the mixed-scale bank.rescale N times: the body for `rocprofv3 --kernel-trace --stats --`. Needs a GPU."""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_m2f_match import wall  # noqa: E402

B, OBJ_H, OBJ_W, N_OBJ = 16, 480, 640, 32
MAP_H, MAP_W, CROP = 1024, 2048, (700, 700)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20, help="launches between two device events")
    ap.add_argument("--loop", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_object_bank needs an MI355X: there is no CPU measurement path")
    from multishiftseg_amd import _lib_obj as L
    from multishiftseg_amd import datapath as D
    from multishiftseg_amd.object_bank import ObjectBank
    peak = json.load(open(os.path.join(ROOT, "profiles", "r06", "measured_peaks.json")))["stream_write_only_GBs"]
    g = torch.Generator().manual_seed(0)
    objs = [(torch.randint(0, 256, (OBJ_H, OBJ_W, 3), generator=g, dtype=torch.uint8), torch.full((OBJ_H, OBJ_W), 7, dtype=torch.uint8))
            for _ in range(N_OBJ)]
    bank = ObjectBank(objs, device="cuda")
    rng = random.Random(0)
    batches = {"scale_1.0": [(rng.randint(0, N_OBJ - 1), 1.0) for _ in range(B)],
               "scale_0.5": [(rng.randint(0, N_OBJ - 1), 0.5) for _ in range(B)],
               "scale_mix": [(rng.randint(0, N_OBJ - 1), rng.choice(D.OOD_SCALES)) for _ in range(B)]}
    if args.loop:
        for _ in range(args.loop):
            bank.rescale(batches["scale_mix"])
        torch.cuda.synchronize()
        return
    maps = (torch.randint(0, 256, (B, MAP_H, MAP_W, 3), generator=g, dtype=torch.uint8).cuda(),
            torch.randint(0, 256, (B, MAP_H, MAP_W, 3), generator=g, dtype=torch.uint8).cuda(),
            torch.randint(0, 19, (B, MAP_H, MAP_W), generator=g, dtype=torch.uint8).cuda(),
            torch.randint(0, 19, (B, MAP_H, MAP_W), generator=g, dtype=torch.uint8).cuda())
    res = {"device": torch.cuda.get_device_name(0), "B": B, "object": [OBJ_H, OBJ_W], "bank_objects": N_OBJ, "resident_bytes": bank.resident_bytes,
           "maps": [MAP_H, MAP_W], "crop": list(CROP), "launches_per_window": args.inner, "write_only_stream_GBs": peak, "batches": {}}
    for name, picks in batches.items():
        boxes = [bank.bbox(k, s) for k, s in picks]
        window_px = sum((y2 - y1) * (x2 - x1) for y1, x1, y2, x2 in boxes)
        img, mask = bank.rescale(picks)
        jobs = torch.tensor([bank._source(k, s) + (y1, x1, y2 - y1, x2 - x1) for (k, s), (y1, x1, y2, x2) in zip(picks, boxes)], dtype=torch.int32).cuda()

        def launch():
            for _ in range(args.inner):
                L.call("mss_obj_rescale_f32", L.ptr(bank.img), L.ptr(bank.mask), bank.pixels, L.ptr(jobs), B, img.shape[1], img.shape[2], L.ptr(img),
                       L.ptr(mask))
        # the two parameter lists of one batch: picks for the bank, and the same objects rescaled beforehand for the host path
        prm_bank, prm_host = [], []
        img_h, mask_h = img.cpu().numpy(), mask.cpu().numpy()
        for b, (pick, (y1, x1, y2, x2)) in enumerate(zip(picks, boxes)):
            bh, bw = y2 - y1, x2 - x1
            base = {"p": min(rng.random(), 0.3), "top": rng.randint(0, MAP_H - CROP[0]), "left": rng.randint(0, MAP_W - CROP[1])}
            geom = (0, 0, bh, bw, rng.randint(0, CROP[0] - bh), rng.randint(0, CROP[1] - bw))
            prm_bank.append(dict(base, pick=pick, geom=geom))
            prm_host.append(dict(base, obj_img=np.ascontiguousarray(img_h[b, :bh, :bw]), obj_mask=np.ascontiguousarray(mask_h[b, :bh, :bw]), geom=geom))
        sides = {"rescale_call_ms": lambda: bank.rescale(picks),
                 "pair_batch_bank_ms": lambda: D.make_pair_batch(*maps, CROP, prm_bank, bank=bank),
                 "pair_batch_host_ms": lambda: D.make_pair_batch(*maps, CROP, prm_host)}
        a, b_ = sides["pair_batch_bank_ms"](), sides["pair_batch_host_ms"]()
        same = bool(torch.equal(a[0], b_[0]) and torch.equal(a[1], b_[1]))
        del a, b_
        times, kernel = {k: [] for k in sides}, []
        for rnd in range(3 + args.rounds):                          # the sides alternate; three warm-up rounds
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            launch()
            e.record()
            torch.cuda.synchronize()
            if rnd >= 3:
                kernel.append(s.elapsed_time(e) / args.inner)
            for k, fn in sides.items():
                t = wall(fn)
                if rnd >= 3:
                    times[k].append(t)
        r = {"scales": [s for _, s in picks], "window_pixels": window_px, "bytes_written": 13 * window_px, "OHmax_OWmax": list(img.shape[1:3]),
             "host_upload_bytes_before": 13 * B * int(img.shape[1]) * int(img.shape[2]), "outputs_equal": same,
             "kernel_ms": statistics.median(kernel), "kernel_min_max_ms": [min(kernel), max(kernel)]}
        r["kernel_GBs"] = r["bytes_written"] / (r["kernel_ms"] * 1e-3) / 1e9
        r["share_of_write_only_stream"] = r["kernel_GBs"] / peak
        r.update({k: statistics.median(v) for k, v in times.items()})
        r.update({k.replace("_ms", "_min_max_ms"): [min(v), max(v)] for k, v in times.items()})
        r["pair_batch_host_over_bank"] = r["pair_batch_host_ms"] / r["pair_batch_bank_ms"]
        res["batches"][name] = r
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
