"""Stage 1 of Mask2Former (train_m2f.py:437-456 before warmup_epoch): m2f_trainer.M2FStage1Step on the full-size model -- R50,
six encoder layers, nine decoder layers, 100 queries, 19 classes, synthetic weights -- and, timed apart, its tail: forward and
backward of kernels.m2f_semantic_inference (upsample of the mask logits to the padded image, the class mix of both heads, the crop,
1 - max_c; backward to pred_logits_ood) on the step's own frozen tensors.

    python tools/bench_m2f_stage1.py [--shape c4|eval] [--rounds 7] [--out profiles/m2f_stage1/bench_c4.json] [--loop N]

Shapes: c4 = 16 crops of 700 x 700 (padded to 704 x 704), eval = 2 images of 1024 x 2048. Times are host clocks around work that
ends in a device synchronise, medians over --rounds after two warm-up rounds; the launches of the tail are also timed one by one
with device events. The bytes are what the algorithm moves, counted from the shapes below (U = the upsampled logits
[B, Hp, Wp, ldq]); bytes / tail time is compared with the copy peak of profiles/r06/measured_peaks.json. --loop N only repeats the
tail N times: the body for `rocprofv3 --kernel-trace --stats -- python tools/bench_m2f_stage1.py --loop 5`. Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_m2f_match import device_ms, wall  # noqa: E402

SHAPES = {"c4": dict(B=16, size=(700, 700)), "eval": dict(B=2, size=(1024, 2048))}
GEOM = dict(num_classes=19, hidden_dim=256, num_queries=100, nheads=8, dim_feedforward=2048, dec_layers=9, pre_norm=False, mask_dim=256,
            enforce_input_project=False)
RCL = {"ce_weights": [0, 0], "inoutaug_contras_margins_tri": [0.7, 0.5, 0.2]}          # M2F.yaml:29-33


def build_model():
    import ref_resnet as RR
    import ref_transformer_decoder as RT
    from multishiftseg_amd import MaskFormer, MultiScaleMaskedTransformerDecoder_GMA, build_resnet_backbone
    from multishiftseg_amd.msdeformattn_decoder import MSDeformAttnPixelDecoder
    torch.manual_seed(0)
    backbone = RR.randomize_(build_resnet_backbone(), 7)
    decoder = MSDeformAttnPixelDecoder(backbone.output_shape(), transformer_dropout=0.0, transformer_nheads=8, transformer_dim_feedforward=1024,
                                       transformer_enc_layers=6, conv_dim=256, mask_dim=256, norm="GN",
                                       transformer_in_features=["res3", "res4", "res5"], common_stride=4)
    predictor = MultiScaleMaskedTransformerDecoder_GMA(256, True, **GEOM)
    predictor.load_state_dict(RT.synth_state_dict(41), strict=True)
    return MaskFormer(backbone, decoder, predictor).cuda().eval()


def tail_bytes(B, Q, C, ldq, low, padded, size):
    """Bytes the tail's launches read and write, per launch and in all, from the shapes alone."""
    (hm, wm), (Hp, Wp), (H, W) = low, padded, size
    lo, U, mix = B * hm * wm * ldq * 4, B * Hp * Wp * ldq * 4, B * C * Hp * Wp * 4
    sem, score = B * min(C, 19) * H * W * 4, B * H * W * 4
    fwd = {"upsample": lo + U, "mix_forward_sem": U + mix, "mix_forward_ood": U + mix, "crop_logits": mix + sem, "crop_neg_max": mix + score}
    bwd = {"upsample_again": lo + U, "crop_backward": mix + score + mix, "mix_backward_dcls": U + mix}
    return dict(U=U, forward=fwd, backward=bwd, forward_total=sum(fwd.values()), backward_total=sum(bwd.values()),
                total=sum(fwd.values()) + sum(bwd.values()), passes_over_U=(2 + 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="c4", choices=sorted(SHAPES))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--loop", type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_m2f_stage1 needs an MI355X: there is no CPU measurement path")
    from multishiftseg_amd import M2FStage1Step
    from multishiftseg_amd import kernels as K
    from multishiftseg_amd.loss import RelContrastiveLoss
    cfg = SHAPES[args.shape]
    B, (H, W) = cfg["B"], cfg["size"]
    model = build_model()
    g = torch.Generator(device="cuda").manual_seed(0)
    images = torch.rand((B, 3, H, W), device="cuda", generator=g)
    target = torch.randint(0, 19, (B, H, W), device="cuda", generator=g)
    target[:, :8] = 255
    target[B // 2:, H // 3:H // 2, W // 3:W // 2] = 254                        # OOD objects in the augmented half
    step = M2FStage1Step(model, RelContrastiveLoss(RCL, pairing="device"))

    # the tail's own inputs: what the predictor hands to m2f_semantic_inference in this step
    with torch.no_grad():
        x = model.pad(images)
        feats = model.backbone(x)
        mf, _, ms = model.sem_seg_head.pixel_decoder.forward_features(feats)
        pred = model.sem_seg_head.predictor
        _, _, lg, _ = pred._forward_frozen(ms, mf, False)
        out = pred(ms, mf, None)
    del feats, mf, ms
    Hp, Wp = x.shape[-2:]
    cls, cls_ood = out["pred_logits"], out["pred_logits_ood"].clone().requires_grad_(True)
    Q, C = cls.shape[1], cls.shape[2] - 1
    _, hm, wm, ldq = lg.shape
    gscore = torch.randn((B, H, W), device="cuda", generator=g)

    def tail(backward=True):
        sem, score = K.m2f_semantic_inference(cls, lg, (Hp, Wp), (H, W), class_logits_ood=cls_ood, Q=Q)
        if backward:
            score.backward(gscore)
            cls_ood.grad = None

    if args.loop:
        for _ in range(args.loop):
            tail()
        torch.cuda.synchronize()
        return
    sides = {"step_ms": lambda: step(images, target.clone()), "tail_forward_ms": lambda: tail(False), "tail_forward_backward_ms": tail}
    times = {k: [] for k in sides}
    torch.cuda.reset_peak_memory_stats()
    for r in range(2 + args.rounds):
        for k, fn in sides.items():
            t = wall(fn)
            if r >= 2:
                times[k].append(t)
    res = dict(device=torch.cuda.get_device_name(0), shape=args.shape, B=B, Q=Q, C=C, ldq=ldq, low=[hm, wm], padded=[Hp, Wp], size=[H, W],
               rounds=args.rounds, budget_bytes=K.stage1_budget(), chunks=K.stage1_chunks(B, Hp, Wp, ldq),
               peak_memory_bytes=torch.cuda.max_memory_allocated())
    res.update({k: statistics.median(v) for k, v in times.items()})
    res.update({k.replace("_ms", "_min_max_ms"): [min(v), max(v)] for k, v in times.items()})
    res["tail_share_of_step"] = res["tail_forward_backward_ms"] / res["step_ms"]
    res["bytes"] = tail_bytes(B, Q, C, ldq, (hm, wm), (Hp, Wp), (H, W))
    peaks = json.load(open(os.path.join(ROOT, "profiles", "r06", "measured_peaks.json")))
    res["tail_GBs"] = res["bytes"]["total"] / res["tail_forward_backward_ms"] / 1e6
    res["copy_peak_GBs"] = peaks["stream_copy_GBs"]
    res["tail_share_of_copy_peak"] = res["tail_GBs"] / peaks["stream_copy_GBs"]

    # the launches one by one, on the first chunk of images (what one pass of the chunk loop runs)
    n = res["chunks"][0][1]
    lgc, clsc, oodc = lg[:n].contiguous(), cls[:n].contiguous(), cls_ood.detach()[:n].contiguous()
    U = K.upsample_bilinear_nhwc(lgc, (Hp, Wp))
    mix, prob = K.m2f_class_mix(oodc, U, pixel_major=True, Q=Q)
    dmix = K.m2f_mix_upsample_backward(mix, (Hp, Wp), (H, W), dscore=gscore[:n].contiguous())
    dev = {"images": n}
    dev["upsample"] = device_ms(lambda: K.upsample_bilinear_nhwc(lgc, (Hp, Wp)), args.rounds)
    dev["mix_forward"] = device_ms(lambda: K.m2f_class_mix(clsc, U, pixel_major=True, Q=Q), args.rounds)
    dev["crop_logits"] = device_ms(lambda: K.m2f_mix_upsample(mix, (Hp, Wp), (H, W), "logits"), args.rounds)
    dev["crop_neg_max"] = device_ms(lambda: K.m2f_mix_upsample(mix, (Hp, Wp), (H, W), "neg_max"), args.rounds)
    dev["crop_backward"] = device_ms(lambda: K.m2f_mix_upsample_backward(mix, (Hp, Wp), (H, W), dscore=gscore[:n].contiguous()), args.rounds)
    both = {"mix_backward_dcls_only": [], "mix_backward_with_dmasks": []}
    for _ in range(args.rounds):                                               # the two forms of the mix backward, alternating
        both["mix_backward_dcls_only"].append(device_ms(lambda: K.m2f_class_mix_backward(dmix, prob, oodc, U, pixel_major=True, Q=Q, want_dmasks=False), 1))
        both["mix_backward_with_dmasks"].append(device_ms(lambda: K.m2f_class_mix_backward(dmix, prob, oodc, U, pixel_major=True, Q=Q), 1))
    dev.update({k: statistics.median(v) for k, v in both.items()})
    res["device_ms_first_chunk"] = dev
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
