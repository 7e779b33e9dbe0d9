"""Forward (and, with --backward, forward + backward) time of the GMA transformer decoder: the HIP module (multishiftseg_amd/transformer_decoder.py) against the fp32
stock-torch restatement of the reference (tests/ref_transformer_decoder.py) on the same GPU.

    python tools/bench_transformer_decoder.py [--out profiles/transformer_decoder/bench.json] [--points c4_b1,c4_b16,c5_b1]
    python tools/bench_transformer_decoder.py --one c5_b1          # one forward of the module (for rocprofv3 --kernel-trace)
    python tools/bench_transformer_decoder.py --backward           # forward + backward: set_trainable() module against helper autograd
    python tools/bench_transformer_decoder.py --attn-backward      # the masked attention's backward kernels alone, with achieved GB/s

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


def _scalar(out):
    """One scalar that pulls on every head of the last step and on every auxiliary mask."""
    loss = out["pred_logits"].sum() + out["pred_logits_ood"].sum() + out["pred_masks"].mean()
    for a in out["aux_outputs"]:
        loss = loss + a["pred_logits"].sum() + a["pred_logits_ood"].sum() + a["pred_masks"].mean()
    return loss


def setup(point, seed=21, backward=False):
    from multishiftseg_amd import MultiScaleMaskedTransformerDecoder_GMA
    B, sizes, fsize = POINTS[point]
    x, feat = R.synth_inputs(211, B, sizes, fsize)
    xs, ft = [torch.from_numpy(v).cuda() for v in x], torch.from_numpy(feat).cuda()
    sd = R.synth_state_dict(seed, device="cuda")
    m = MultiScaleMaskedTransformerDecoder_GMA(256, True, **GEOM)
    m.load_state_dict(sd, strict=True)
    m = m.cuda().eval()
    if backward:
        m.set_trainable()
        for k, t in sd.items():
            t.requires_grad_("fusion_layer" not in k)
        for t in xs + [ft]:
            t.requires_grad_(True)
        leaves = [t for t in sd.values() if t.requires_grad] + xs + [ft]

        def helper_fb():
            for t in leaves:
                t.grad = None
            _scalar(R.decoder_forward(sd, xs, ft, 9)).backward()

        def module_fb():
            m.zero_grad(set_to_none=True)
            for t in xs + [ft]:
                t.grad = None
            _scalar(m(xs, ft)).backward()
        return helper_fb, module_fb

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


def attn_backward(point, iters=20):
    """The attention backward alone at the point's finest level (A = 2, masked at 50 %): milliseconds per call and the achieved
    bandwidth over the compulsory traffic (k, v read once by each of the two kernels, dk and dv written once)."""
    from multishiftseg_amd import kernels as K
    B, sizes, _ = POINTS[point]
    NK, Q, A = sizes[-1][0] * sizes[-1][1], 100, 2
    g = torch.Generator(device="cuda").manual_seed(1)
    q = torch.randn((B * Q, A * 256), device="cuda", generator=g)
    k = torch.randn((B * NK, A * 256), device="cuda", generator=g)
    v = torch.randn((B * NK, A * 256), device="cuda", generator=g)
    cot = torch.randn((B * Q, A * 256), device="cuda", generator=g)
    logits = torch.randn((B, sizes[-1][0], sizes[-1][1], Q), device="cuda", generator=g)
    bits, allowed = K.m2f_attn_mask_bits(logits, Q, sizes[-1])
    out, lse = K.m2f_masked_attention_lse(q, k, v, B, Q, NK, A=A, bits=bits, allowed=allowed)
    run = lambda: K.m2f_masked_attention_backward(q, k, v, out, lse, cot, B, Q, NK, A=A, bits=bits, allowed=allowed)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ts = [timed(run) for _ in range(iters)]
    ms = statistics.median(ts)
    nbytes = 6.0 * B * NK * A * 256 * 4
    return {"point": point, "attn_backward_ms": ms, "ms_min_max": [min(ts), max(ts)], "bytes": nbytes, "GBps": nbytes / ms / 1e6,
            "flop": 2.0 * 224 * B * NK * Q * 8 * A, "keys": NK, "B": B}


def bench(point, warmup=5, rounds=20, backward=False):
    helper, module = setup(point, backward=backward)
    for _ in range(warmup):
        helper()
        module()
    torch.cuda.synchronize()
    th, tm = [], []
    for _ in range(rounds):
        th.append(timed(helper))
        tm.append(timed(module))
    res = {"point": point, "mode": "forward+backward" if backward else "forward", "helper_ms": statistics.median(th), "module_ms": statistics.median(tm),
           "helper_ms_min_max": [min(th), max(th)], "module_ms_min_max": [min(tm), max(tm)],
           "helper_peak_mib": peak(helper), "module_peak_mib": peak(module), "rounds": rounds, "warmup": warmup}
    res["speedup"] = res["helper_ms"] / res["module_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--points", default="c4_b1,c4_b16,c5_b1")
    ap.add_argument("--one", default=None, help="run one warmed-up forward of the module at this point and exit")
    ap.add_argument("--backward", action="store_true", help="time forward + backward (the module with set_trainable())")
    ap.add_argument("--attn-backward", action="store_true", help="time the masked attention's backward kernels alone")
    ap.add_argument("--rounds", type=int, default=20)
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
        r = attn_backward(p) if args.attn_backward else bench(p, rounds=args.rounds, backward=args.backward)
        results.append(r)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
