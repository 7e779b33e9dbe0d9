"""Times the 7x7 stem kernel and the whole ResNet-50 backbone forward on the MI355X against stock torch on the same device.

  stem:     kernels.stem7_conv's convolution launch alone (image already NHWC with its zero channel; folded norm + ReLU fused) and
            the whole wrapper (NCHW -> NHWC + convolution), against F.conv2d for the same layer and F.relu(F.batch_norm(F.conv2d)).
  backbone: ResNet.forward against the tests/ref_resnet.py restatement in float32 with stock torch.

  --backward: forward + backward of the trainable backbone (ResNet.set_trainable(), the faithful stage-2 freezing pattern
            freeze(1, norms=True): the 52 res2..res5 convolution weights) against stock-torch float32 autograd of the same
            restatement on the same device, at 8 x 3 x 384 x 768 (the reference's 380 x 760 crop padded to 32, batch 8) and
            2 x 3 x 1024 x 2048; and, separately, the six stride-2 data gradients (conv2 and shortcut of res3.0 / res4.0 / res5.0) on
            kernels.conv2d_dgrad_s2 against the zero-insertion form through the stride-1 kernel (with and without its insertion pass).
  --backward --stem: the stem weight trained too (set_trainable(stem=True), freeze(0, norms=True): 53 weights). Per size: the stem
            backward alone -- the launch of csrc/stem7_wgrad.hip with the max-pool and ReLU backward fused (image already NHWC), its
            plain form on a given dz, and the whole kernels.stem7_wgrad wrapper -- against stock torch float32 on the same device
            (backward of max_pool2d(relu(conv2d)) to the weight: conv weight gradient + max-pool backward + ReLU gate); then forward +
            backward with 53 weights, with the stem frozen (52: the calls of freeze(1, norms=True)) and stock torch with 53, alternating.
            The strided data gradients are not repeated.

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
BACKWARD_SIZES = [(8, 384, 768), (2, 1024, 2048)]


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


def backward_bench(args):
    import ref_resnet as R
    from multishiftseg_amd import build_resnet_backbone, kernels as K
    sizes = BACKWARD_SIZES if args.sizes is None else [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
    if args.stem:
        return stem_backward_bench(args, sizes)
    model = R.randomize_(build_resnet_backbone(), 7).eval().cuda().set_trainable().freeze(1, norms=True)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    params = [p for _, p in named]
    sd = R.cast(model.state_dict(), torch.float32)
    leaves = [sd[n].requires_grad_(True) for n, _ in named]                 # the same 52 tensors, stock torch's own copies
    names = ("res2", "res3", "res4", "res5")
    result = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, pattern="freeze(1, norms=True): 52 convolution weights", shapes=[])
    for n, h, w in sizes:
        img = torch.randn((n, 3, h, w), device="cuda")
        with torch.no_grad():
            gm = [torch.randn_like(t) for t in model(img).values()]

        def hip_step():
            return torch.autograd.grad(list(model(img).values()), params, gm)

        def torch_step():
            out = R.resnet50(img, sd)
            return torch.autograd.grad([out[k] for k in names], leaves, gm)

        def hip_forward():
            with torch.no_grad():
                return model(img)
        step = timed({"resnet50_hip_fwd_bwd": hip_step, "resnet50_torch_f32_fwd_bwd": torch_step, "resnet50_hip_fwd": hip_forward},
                     args.rounds, iters=3, warm=2)
        ours, ref = hip_step(), torch_step()
        diffs = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(ours, ref)]
        del ours, ref
        # the six strided data gradients alone: the parity-class kernel against zero insertion + the stride-1 kernel
        strided = []
        for stage in ("res3", "res4", "res5"):
            blk = getattr(model, stage)[0]
            div = model._out_feature_strides[stage] // 2                       # the block's input stride
            ih, iw = h // div, w // div
            for conv in (blk.conv2, blk.shortcut):
                cz, cx, r, _ = conv.weight.shape
                pw = K.packed(conv.weight, flip=True)
                dz = K.Act(torch.randn((n, ih // 2, iw // 2, cz), device="cuda"))
                up = K.Act.zeros(n, ih, iw, cz, "cuda")

                def insert():
                    up.buf.zero_()
                    up.buf[:, ::2, ::2, :] = dz.buf
                t = timed({"dgrad_s2": lambda: K.conv2d_dgrad_s2(dz, pw, (ih, iw)),
                           "zero_insertion_product": lambda: K.conv2d(up, pw, pad=r // 2),
                           "zero_insertion_with_pass": lambda: (insert(), K.conv2d(up, pw, pad=r // 2))}, args.rounds, iters=10, warm=3)
                insert()
                diff = float((K.conv2d_dgrad_s2(dz, pw, (ih, iw)).buf - K.conv2d(up, pw, pad=r // 2).buf).abs().max())
                flop = 2.0 * n * (ih // 2) * (iw // 2) * cz * cx * r * r
                strided.append(dict(layer=f"{stage}.0.{'conv2' if r == 3 else 'shortcut'}", dz=[n, ih // 2, iw // 2, cz], dx=[n, ih, iw, cx],
                                    kernel=r, TFLOP=flop / 1e12, times=t, useful_TFLOP_per_s=flop / t["dgrad_s2"]["median_ms"] / 1e9,
                                    max_abs_diff_vs_zero_insertion=diff))
                del dz, up
        entry = dict(shape=[n, 3, h, w], step=step,
                     hip_over_torch=step["resnet50_hip_fwd_bwd"]["median_ms"] / step["resnet50_torch_f32_fwd_bwd"]["median_ms"],
                     hip_fwd_bwd_over_hip_fwd=step["resnet50_hip_fwd_bwd"]["median_ms"] / step["resnet50_hip_fwd"]["median_ms"],
                     weight_grad_rel_max_diff_vs_torch_f32=dict(max=max(diffs), median=statistics.median(diffs)),
                     strided_dgrads=strided,
                     strided_dgrads_ms=dict(dgrad_s2=sum(e["times"]["dgrad_s2"]["median_ms"] for e in strided),
                                            zero_insertion_product=sum(e["times"]["zero_insertion_product"]["median_ms"] for e in strided),
                                            zero_insertion_with_pass=sum(e["times"]["zero_insertion_with_pass"]["median_ms"] for e in strided)))
        result["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        del img, gm
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


def stem_backward_bench(args, sizes):
    import ctypes
    import ref_resnet as R
    from multishiftseg_amd import _lib, build_resnet_backbone, kernels as K
    from multishiftseg_amd.resnet import _folded
    model = R.randomize_(build_resnet_backbone(), 7).eval().cuda().set_trainable(stem=True).freeze(0, norms=True)
    named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
    params = [p for _, p in named]
    stem_w = model.stem.conv1.weight
    assert len(params) == 53 and params[0] is stem_w
    sd = R.cast(model.state_dict(), torch.float32)
    leaves = [sd[n].requires_grad_(True) for n, _ in named]
    names = ("res2", "res3", "res4", "res5")
    result = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, pattern="freeze(0, norms=True), set_trainable(stem=True): 53 convolution weights",
                  shapes=[])
    for n, h, w in sizes:
        img = torch.randn((n, 3, h, w), device="cuda")
        oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        ph, pw = (oh - 1) // 2 + 1, (ow - 1) // 2 + 1
        # ---- the stem backward alone
        with torch.no_grad():
            a0 = K.stem7_conv(img, stem_w, _folded(model.stem.conv1), relu=True)
        gp = K.Act(torch.randn((n, ph, pw, 64), device="cuda"))
        dz = K.Act(torch.randn((n, oh, ow, 64), device="cuda"))
        x4 = K.image_to_nhwc(img, Cp=4)
        dwp = torch.empty((49, 64, 4), device="cuda")

        def launch(dy, res):
            a = _lib.MssConvArgs()
            a.x = x4.ptr
            a.N, a.H, a.W, a.C, a.ldx = n, h, w, 4, 4
            a.OH, a.OW, a.K, a.Kpad = oh, ow, 64, 64
            a.R, a.S, a.stride, a.dil, a.pad = 7, 7, 2, 1, 3
            if res is not None:
                a.res, a.ldres, a.res_mask = res.ptr, res.ld, 1
            nbytes = _lib.value("mss_conv2d_wgrad_workspace_bytes", ctypes.byref(a), 4)
            ws = torch.empty(max(nbytes, 4) // 4, device="cuda")
            plan = _lib.MssWgradPlan()
            assert _lib.value("mss_conv2d_wgrad_plan", ctypes.byref(a), dy.ptr, dy.ld, _lib.ptr(dwp), 4, nbytes, 0, ctypes.byref(plan)) == 0
            return (lambda: _lib.call("mss_conv2d_wgrad_f32", ctypes.byref(a), dy.ptr, dy.ld, _lib.ptr(dwp), 4, _lib.ptr(ws), nbytes)), plan, a
        fused, plan, keep1 = launch(gp, a0)
        plain, _, keep2 = launch(dz, None)
        wt = stem_w.detach().clone().requires_grad_(True)
        y = F.max_pool2d(F.relu(F.conv2d(img, wt, None, 2, 3)), 3, 2, 1)
        gy = gp.buf.permute(0, 3, 1, 2).contiguous()
        stem = timed({"stem7_wgrad_pool_kernel": fused, "stem7_wgrad_plain_kernel": plain, "stem7_wgrad_wrapper": lambda: K.stem7_wgrad(img, gp, a0),
                      "torch_f32_pool_relu_conv_backward": lambda: torch.autograd.grad(y, wt, gy, retain_graph=True)}, args.rounds, iters=20, warm=3)
        m = float(n * oh * ow)
        issued, useful = 2.0 * m * 64 * 7 * 8 * 4, 2.0 * m * 64 * 147
        nbytes = 4.0 * n * (h * w * 4 + oh * ow * 64 + ph * pw * 64) + 2.0 * plan.ws_bytes
        for k in ("stem7_wgrad_pool_kernel", "stem7_wgrad_plain_kernel"):
            stem[k].update(issued_TFLOP_per_s=issued / stem[k]["median_ms"] / 1e9, useful_TFLOP_per_s=useful / stem[k]["median_ms"] / 1e9)
        stem["stem7_wgrad_pool_kernel"].update(TB_per_s=nbytes / stem["stem7_wgrad_pool_kernel"]["median_ms"] / 1e9, model_bytes=nbytes)
        del y, wt, gy, dz, gp, a0, x4
        torch.cuda.empty_cache()
        # ---- forward + backward: 53 weights, 52 (the stem frozen), stock torch with 53
        with torch.no_grad():
            gm = [torch.randn_like(t) for t in model(img).values()]

        def hip_step():
            return torch.autograd.grad(list(model(img).values()), params, gm)

        def hip_step_frozen_stem():
            stem_w.requires_grad_(False)
            try:
                return torch.autograd.grad(list(model(img).values()), params[1:], gm)
            finally:
                stem_w.requires_grad_(True)

        def torch_step():
            out = R.resnet50(img, sd)
            return torch.autograd.grad([out[k] for k in names], leaves, gm)
        step = timed({"resnet50_hip_fwd_bwd_53": hip_step, "resnet50_hip_fwd_bwd_52": hip_step_frozen_stem, "resnet50_torch_f32_fwd_bwd_53": torch_step},
                     args.rounds, iters=3, warm=2)
        ours, ref = hip_step(), torch_step()
        diffs = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(ours, ref)]
        del ours, ref
        entry = dict(shape=[n, 3, h, w], plan=dict(splits=plan.splits, rows_per_split=plan.rows_per_split, ws_bytes=plan.ws_bytes, reduce_group=plan.reduce_group),
                     stem_backward=stem,
                     stem_pool_kernel_over_torch=stem["stem7_wgrad_pool_kernel"]["median_ms"] / stem["torch_f32_pool_relu_conv_backward"]["median_ms"],
                     step=step, hip53_over_hip52=step["resnet50_hip_fwd_bwd_53"]["median_ms"] / step["resnet50_hip_fwd_bwd_52"]["median_ms"],
                     hip53_over_torch53=step["resnet50_hip_fwd_bwd_53"]["median_ms"] / step["resnet50_torch_f32_fwd_bwd_53"]["median_ms"],
                     stem_weight_grad_rel_max_diff_vs_torch_f32=diffs[0],
                     weight_grad_rel_max_diff_vs_torch_f32=dict(max=max(diffs), median=statistics.median(diffs)))
        result["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        del img, gm, keep1, keep2
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--backward", action="store_true", help="time forward + backward and the strided data gradients instead")
    ap.add_argument("--stem", action="store_true", help="with --backward: train the stem weight too; times the stem backward alone and the step with and without it")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sizes", default=None, help="e.g. 1x64x96,2x70x100 (default: the two sizes the reference trains and tests at)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_m2f_backbone.py measures on the GPU only")
    if args.stem and not args.backward:
        raise SystemExit("--stem goes with --backward")
    if args.backward:
        return backward_bench(args)
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
