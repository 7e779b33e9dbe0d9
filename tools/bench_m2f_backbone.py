"""Times the 7x7 stem kernel and the whole ResNet-50 backbone forward on the MI355X against stock torch on the same device.

  stem:     kernels.stem7_conv's convolution launch alone (image already NHWC with its zero channel; folded norm + ReLU fused) and
            the whole wrapper (NCHW -> NHWC + convolution), against F.conv2d for the same layer and F.relu(F.batch_norm(F.conv2d)).
  backbone: ResNet.forward against the tests/ref_resnet.py restatement in float32 with stock torch.

Each pair alternates inside one process: per round every contender runs `iters` times between two device events; the figure is the
median over the rounds, with min and max beside it. Every shape is warmed first. The outputs of both sides are compared at the timed
size. Reported, not gated: python tools/bench_m2f_backbone.py --out profiles/m2f_backbone/bench.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch                                    # noqa: E402
import torch.nn.functional as F                 # noqa: E402

SIZES = [(2, 1024, 2048), (16, 704, 704)]


def timed(fns, rounds, iters, warm):
    """{name: (median, min, max)} in ms per call; the contenders alternate round by round."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(iters):
                fn()
            e.record()
            e.synchronize()
            ms[name].append(s.elapsed_time(e) / iters)
    return {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default=None, help="e.g. 1x64x96,2x70x100 (default: the two sizes the reference trains and tests at)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_m2f_backbone.py measures on the GPU only")
    import ref_resnet as R
    from multishiftseg_amd import build_resnet_backbone, kernels as K
    from multishiftseg_amd.resnet import _folded
    sizes = SIZES if args.sizes is None else [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
    model = R.randomize_(build_resnet_backbone(), 7).eval().cuda()
    for p in model.parameters():
        p.requires_grad_(False)
    sd = R.cast(model.state_dict(), torch.float32)
    conv1 = model.stem.conv1
    bn = conv1.norm
    result = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, shapes=[])
    with torch.no_grad():
        for n, h, w in sizes:
            img = torch.randn((n, 3, h, w), device="cuda")
            oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
            x4, pw, aff = K.image_to_nhwc(img, Cp=4), K.packed_stem7(conv1.weight), _folded(conv1)
            out = K.Act.empty(n, oh, ow, 64, img.device)

            def stem_kernel():
                K._conv_launch(x4, pw, out, oh, ow, 2, 1, 3, None, False, aff, True, None)

            def torch_layer():
                return F.relu(F.batch_norm(F.conv2d(img, conv1.weight, None, 2, 3), bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps))
            stem = timed({"stem7_kernel": stem_kernel, "stem7_conv_wrapper": lambda: K.stem7_conv(img, conv1.weight, aff),
                          "torch_conv2d": lambda: F.conv2d(img, conv1.weight, None, 2, 3), "torch_conv2d_norm_relu": torch_layer},
                         args.rounds, iters=50, warm=5)
            flop = 2.0 * n * oh * ow * 64 * 147
            nbytes = 4.0 * n * (h * w * 4 + oh * ow * 64)
            stem["stem7_kernel"].update(useful_TFLOP_per_s=flop / stem["stem7_kernel"]["median_ms"] / 1e9,
                                        issued_TFLOP_per_s=flop * 196 / 147 / stem["stem7_kernel"]["median_ms"] / 1e9,
                                        TB_per_s=nbytes / stem["stem7_kernel"]["median_ms"] / 1e9)
            stem_kernel()
            stem_diff = float((out.nchw() - torch_layer()).abs().max())
            back = timed({"resnet50_hip": lambda: model(img), "resnet50_torch_f32": lambda: R.resnet50(img, sd)}, args.rounds, iters=5, warm=2)
            ours, ref = model(img), R.resnet50(img, sd)
            diffs = {k: float((ours[k] - ref[k]).abs().max() / ref[k].abs().max()) for k in ours}
            entry = dict(shape=[n, 3, h, w], stem=stem, stem_max_abs_diff_vs_torch_f32=stem_diff,
                         stem_kernel_over_torch_conv2d=stem["stem7_kernel"]["median_ms"] / stem["torch_conv2d"]["median_ms"],
                         backbone=back, backbone_hip_over_torch=back["resnet50_hip"]["median_ms"] / back["resnet50_torch_f32"]["median_ms"],
                         backbone_rel_max_diff_vs_torch_f32=diffs)
            result["shapes"].append(entry)
            print(json.dumps(entry))
            del img, x4, out, ours, ref
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
