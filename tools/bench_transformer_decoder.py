"""Forward time of the GMA transformer decoder: the HIP module (multishiftseg_amd/transformer_decoder.py) against the fp32
stock-torch restatement of the reference (tests/ref_transformer_decoder.py) on the same GPU.

    python tools/bench_transformer_decoder.py [--out profiles/transformer_decoder/bench.json] [--points c4_b1,c4_b16,c5_b1]
    python tools/bench_transformer_decoder.py --one c5_b1          # one forward of the module (for rocprofv3 --kernel-trace)

A and B alternate inside one process (5 warm-up rounds, then 20 timed rounds of helper, module, helper, module ...; median
per side; device events around each forward, which ends in a synchronise). Peak memory is torch's allocator peak over one
forward of each side. Points: C4 = 704 x 704 (levels 22^2 / 44^2 / 88^2, 176^2 mask features) at B = 1 and 16, C5 = 1024 x 2048
(32x64 / 64x128 / 128x256, 256x512) at B = 1. Weights and inputs are synthetic (synth.gen_tensor, a numpy seed). Needs a GPU:
there is no CPU measurement path.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_transformer_decoder as R  # noqa: E402

POINTS = {
    "c4_b1": (1, [(22, 22), (44, 44), (88, 88)], (176, 176)),
    "c4_b16": (16, [(22, 22), (44, 44), (88, 88)], (176, 176)),
    "c5_b1": (1, [(32, 64), (64, 128), (128, 256)], (256, 512)),
}
GEOM = dict(num_classes=19, hidden_dim=256, num_queries=100, nheads=8, dim_feedforward=2048, dec_layers=9, pre_norm=False,
            mask_dim=256, enforce_input_project=False)


def setup(point, seed=21):
    from multishiftseg_amd import MultiScaleMaskedTransformerDecoder_GMA
    B, sizes, fsize = POINTS[point]
    x, feat = R.synth_inputs(211, B, sizes, fsize)
    xs, ft = [torch.from_numpy(v).cuda() for v in x], torch.from_numpy(feat).cuda()
    sd = R.synth_state_dict(seed, device="cuda")
    m = MultiScaleMaskedTransformerDecoder_GMA(256, True, **GEOM)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()

    def helper():
        with torch.no_grad():
            return R.decoder_forward(sd, xs, ft, 9)["pred_logits_ood"]

    def module():
        with torch.no_grad():
            return m(xs, ft)["pred_logits_ood"]
    return helper, module


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def bench(point, warmup=5, rounds=20):
    helper, module = setup(point)
    for _ in range(warmup):
        helper()
        module()
    torch.cuda.synchronize()
    th, tm = [], []
    for _ in range(rounds):
        th.append(timed(helper))
        tm.append(timed(module))
    res = {"point": point, "helper_ms": statistics.median(th), "module_ms": statistics.median(tm),
           "helper_ms_min_max": [min(th), max(th)], "module_ms_min_max": [min(tm), max(tm)],
           "helper_peak_mib": peak(helper), "module_peak_mib": peak(module), "rounds": rounds, "warmup": warmup}
    res["speedup"] = res["helper_ms"] / res["module_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--points", default="c4_b1,c4_b16,c5_b1")
    ap.add_argument("--one", default=None, help="run one warmed-up forward of the module at this point and exit")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_transformer_decoder needs an MI355X: there is no CPU measurement path")
    if args.one:
        _, module = setup(args.one)
        for _ in range(3):
            module()
        torch.cuda.synchronize()
        return
    results = []
    for p in args.points.split(","):
        r = bench(p)
        results.append(r)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
