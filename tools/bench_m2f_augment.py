"""The Mask2Former input path (multishiftseg_amd/m2f_datapath.py over libmss_aug.so) at the size a user runs: one 1024 x 2048
pair, crop 512 x 1024.

  (a) every stage alone on the sample's working set (x float32 [2,3,1024,2048], m uint8 [2,1024,2048]): device events around
      `reps` back-to-back calls after a warm-up, median over `rounds`; the bytes each stage must move (computed here from the
      shapes) over that time, as a rate. That rate includes the launches and allocations of the Python wrapper: it is a
      call rate, not a kernel's share of peak.
  (b) the whole sample with every chain entry applied, and a batch of 8 with seeded decisions (random.seed / torch.manual_seed):
      host clock around a call that ends synchronised.
  (c) beside each, the stock-torch CPU restatement of the same stage / chain (tests/ref_augment.py) on 16 threads.

    python tools/bench_m2f_augment.py [--out profiles/m2f_augment/bench.json] [--rounds 7] [--cpu-rounds 2]

Needs a GPU: there is no CPU measurement path."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W, CROP = 1024, 2048, (512, 1024)


def device_ms(fn, rounds, reps):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) / reps)
    return statistics.median(ts), min(ts), max(ts)


def wall_ms(fn, rounds, sync=True):
    ts = []
    for _ in range(rounds):
        if sync:
            torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-rounds", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_m2f_augment needs an MI355X: there is no CPU measurement path")
    torch.set_num_threads(16)
    import ref_augment as R
    from multishiftseg_amd import m2f_datapath as D

    x, m = R.rand_stack(H, W)
    xd, md = x.cuda(), m.cuda()
    img, gen, tgt, gtg = R.rand_maps(1, H, W)
    maps1 = tuple(t[0].cuda() for t in (img, gen, tgt, gtg))
    px, pm = 2 * 3 * H * W * 4, 2 * H * W                      # bytes of x and of m
    half = (int(H * 0.7), int(W * 0.7))
    out_img = torch.empty((2, 3) + CROP, device="cuda")
    out_tgt = torch.zeros((2,) + CROP, device="cuda", dtype=torch.int64)
    jit = ([2, 0, 3, 1], 1.3, 0.7, 1.4, 0.1)
    # name -> (device call, CPU restatement, bytes the stage must move)
    stages = {
        "load": (lambda: D.load_pair(*maps1, 0.2), lambda: R.load(img[0], gen[0], tgt[0], gtg[0], 0.2), 2 * H * W * 4 + px + pm),
        "stats": (lambda: D.image_stats(xd), lambda: (R.gray(x).mean(dim=(-3, -2, -1)), x.amin(dim=(-2, -1)), x.amax(dim=(-2, -1))), px),
        "color_jitter": (lambda: D.color_jitter(xd.clone(), *jit), lambda: R.color_jitter(x, jit[0], jit[1:]), 3 * px + 2 * px),
        "autocontrast": (lambda: D.autocontrast(xd.clone()), lambda: R.autocontrast(x), 3 * px + 2 * px),
        "gaussian_blur": (lambda: D.gaussian_blur(xd, 2.5), lambda: R.gaussian_blur(x, 2.5), 2 * px),
        "sharpness": (lambda: D.sharpness(xd, 1.5), lambda: R.sharpness(x, 1.5), 2 * px),
        "equalize": (lambda: D.equalize(xd.clone()), lambda: R.equalize(x), 3 * px + 2 * px),
        "resize_0.7": (lambda: D.resize(xd, md, half), lambda: (R.resize(x, half), R.resize_mask(m, half)), int((px + pm) * 1.49)),
        "rotate": (lambda: D.rotate(xd, md, 7.0), lambda: (R.rotate(x, 7.0), R.rotate_mask(m, 7.0)), 2 * (px + pm)),
        "window_flip": (lambda: D.window(xd, md, hflip=True, vflip=True), lambda: R.window(x, m, True, True), 2 * (px + pm)),
        "finish_crop": (lambda: D.finish(xd, md, out_img, out_tgt, 0, True, False, 100, 200, CROP),
                        lambda: R.normalize(R.window(x, m, True, False, 100, 200, CROP)[0]), CROP[0] * CROP[1] * 2 * (12 + 1 + 12 + 8)),
    }
    clone_ms = device_ms(lambda: xd.clone(), args.rounds, args.reps)[0]      # the in-place stages are timed with a copy in front
    res = {"device": torch.cuda.get_device_name(0), "shape": [H, W], "crop": list(CROP), "cpu_threads": torch.get_num_threads(),
           "rounds": args.rounds, "reps": args.reps, "clone_ms": clone_ms, "stages": {}}
    for name, (dev_fn, cpu_fn, nbytes) in stages.items():
        med, lo, hi = device_ms(dev_fn, args.rounds, args.reps)
        cpu = wall_ms(cpu_fn, args.cpu_rounds, sync=False)
        res["stages"][name] = {"device_ms": med, "device_ms_min_max": [lo, hi], "bytes": nbytes, "call_TB_per_s": nbytes / (med * 1e-3) / 1e12,
                               "cpu_ms": cpu[0], "cpu_over_device": cpu[0] / med}
        print(name, json.dumps(res["stages"][name]), flush=True)

    on = tuple((n, 1.0) for n, _ in D.M2F_CHAIN)
    objs = [(torch.rand(120, 160, 3).mul(255).numpy(), torch.full((120, 160), 254, dtype=torch.uint8).numpy())]

    def draw(B, chain):
        random.seed(0)
        torch.manual_seed(0)
        return [D.draw_m2f_sample_params(H, W, CROP, True, objs, lambda o, s: o, chain=chain) for _ in range(B)]

    def cpu_chain(maps, params):
        for b, prm in enumerate(params):
            cx, cm = R.load(maps[0][b], maps[1][b], maps[2][b], maps[3][b], prm["p"])
            for e in prm["entries"]:
                cx, cm = R.apply_entry(cx, cm, e, CROP)
            R.paste(cx[0], cm[0].to(torch.int64), prm["obj_img"], prm["obj_mask"], prm["geom"])
    for tag, B, chain in (("sample_every_entry_on", 1, on), ("batch8_seeded", 8, D.M2F_CHAIN)):
        maps = R.rand_maps(B, H, W)
        dmaps = tuple(t.cuda() for t in maps)
        params = draw(B, chain)
        fn = lambda: D.make_m2f_pair_batch(*dmaps, CROP, params)
        for _ in range(2):
            fn()
        med, lo, hi = wall_ms(fn, args.rounds)
        cpu = wall_ms(lambda: cpu_chain(maps, params), args.cpu_rounds, sync=False)
        res[tag] = {"B": B, "entries_per_sample": [len(p["entries"]) for p in params], "device_ms": med, "device_ms_min_max": [lo, hi],
                    "samples_per_s": B / (med * 1e-3), "cpu_ms": cpu[0], "cpu_samples_per_s": B / (cpu[0] * 1e-3), "cpu_over_device": cpu[0] / med}
        print(tag, json.dumps(res[tag]), flush=True)
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
