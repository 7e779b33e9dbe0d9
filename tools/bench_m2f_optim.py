"""One clipped optimizer step over the real stage-2 tensor list -- every parameter of MultiScaleMaskedTransformerDecoder_GMA and of
MSDeformAttnPixelDecoder at the reference's geometry, taken with named_parameters() -- two ways in one process:

  (a) optim.AdamW: one call of mss_adamw_clip_step_f32 (csrc/m2f_optim.hip): norm launches, one coefficient launch, update launches;
  (b) what the package offered before: torch.nn.utils.clip_grad_norm_ on the device followed by one mss_adam_step_f32 launch per tensor
      (L2-coupled decay: another arithmetic, the same traffic).

    python tools/bench_m2f_optim.py [--out profiles/m2f_optim/bench.json] [--rounds 30]

A and B alternate (5 warm-up rounds, then `rounds` timed rounds a, b, a, b ...; median per side; a host clock around each step, which
ends in a device synchronise, so host launch cost is inside the figure -- it is what the step costs). Gradients are synthetic and
stay allocated. Roofline: the step reads p, g, m, v and writes p, m, v (28 B per element) and the norm pass reads g once more (4 B):
32 B x elements over the measured stream-copy rate of profiles/r06/measured_peaks.json. Needs a GPU: there is no CPU path."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEOM = dict(num_classes=19, hidden_dim=256, num_queries=100, nheads=8, dim_feedforward=2048, dec_layers=9, pre_norm=False,
            mask_dim=256, enforce_input_project=False)
SHAPE = {"res2": (256, 4), "res3": (512, 8), "res4": (1024, 16), "res5": (2048, 32)}
CLIP = 0.01


def build_head():
    from multishiftseg_amd import MultiScaleMaskedTransformerDecoder_GMA
    from multishiftseg_amd.msdeformattn_decoder import MSDeformAttnPixelDecoder, ShapeSpec
    torch.manual_seed(0)
    head = torch.nn.Module()
    head.pixel_decoder = MSDeformAttnPixelDecoder({k: ShapeSpec(*v) for k, v in SHAPE.items()}, transformer_dropout=0.0, transformer_nheads=8,
                                                  transformer_dim_feedforward=1024, transformer_enc_layers=6, conv_dim=256, mask_dim=256, norm="GN",
                                                  transformer_in_features=["res3", "res4", "res5"], common_stride=4)
    head.predictor = MultiScaleMaskedTransformerDecoder_GMA(256, True, **GEOM)
    return head.cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "m2f_optim", "bench.json"))
    ap.add_argument("--rounds", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_m2f_optim needs a GPU: there is no CPU measurement path")
    from multishiftseg_amd import build_m2f_optimizer
    from multishiftseg_amd.optim import Adam, adamw_launches

    head_a, head_b = build_head(), build_head()
    named = [(n, p) for n, p in head_a.named_parameters() if p.requires_grad]
    gen = torch.Generator(device="cuda").manual_seed(1)
    grads = [torch.randn(p.shape, device="cuda", generator=gen) * 1e-2 for _, p in named]
    opt_a = build_m2f_optimizer(head_a, base_lr=1e-5, weight_decay=0.05, clip_value=CLIP)
    params_b = [p for p in head_b.parameters() if p.requires_grad]
    opt_b = Adam(params_b, lr=1e-5, weight_decay=0.05)
    for (_, p), q, g in zip(named, params_b, grads):
        p.grad, q.grad = g, g.clone()

    def step_a():
        return opt_a.step()

    def step_b():
        torch.nn.utils.clip_grad_norm_(params_b, CLIP)
        opt_b.step()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(5):
        timed(step_a), timed(step_b)
    ta, tb = [], []
    for _ in range(args.rounds):
        ta.append(timed(step_a))
        tb.append(timed(step_b))
    elements = sum(p.numel() for _, p in named)
    peaks = json.load(open(os.path.join(ROOT, "profiles", "r06", "measured_peaks.json")))
    roof_ms = 32.0 * elements / (peaks["stream_copy_GBs"] * 1e9) * 1e3
    a_ms, b_ms = statistics.median(ta), statistics.median(tb)
    result = dict(tensors=len(named), elements=elements, launches_new=opt_a.last_launches,
                  launches_predicted=adamw_launches([p.numel() for _, p in named], clip=True), new_ms_median=a_ms, new_ms_min=min(ta), new_ms_max=max(ta),
                  parent_path_ms_median=b_ms, parent_path_ms_min=min(tb), parent_path_ms_max=max(tb), speedup=b_ms / a_ms,
                  roofline_bytes=32 * elements, roofline_stream_GBs=peaks["stream_copy_GBs"], roofline_ms=roof_ms,
                  new_fraction_of_roofline=roof_ms / a_ms, parent_path_fraction_of_roofline=roof_ms / b_ms, rounds=args.rounds,
                  timing="host clock around one step ending in a device synchronise; a and b alternate; medians")
    print(json.dumps(result))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
