"""Writes tests/golden/m2f_transformer_decoder.npz from the reference's MultiScaleMaskedTransformerDecoder_GMA
(lib/network/mask2former/modeling/transformer_decoder/mask2former_transformer_decoder.py:280-573), imported unchanged.

    python tools/gen_golden_transformer_decoder.py --reference DIR

detectron2 / fvcore are absent and un-vendored; the four names the two transformer_decoder files take from them are stubbed
as tools/gen_golden.py:import_reference_decoder does (configurable, Conv2d, c2_xavier_fill) plus detectron2.utils.registry.Registry
for the sibling maskformer_transformer_decoder.py. Geometry: 9 layers, 100 queries, 19 classes, dim_feedforward 2048, mask_dim
256, levels 3x5 / 6x10 / 12x20 with 24x40 mask features (the 96x160 image of m2f_decoder.npz), B = 2. Weights are
synth.gen_tensor(SEED, "m2ftd." + name, shape, gain=1.0); inputs come from a stored numpy seed
(tests/ref_transformer_decoder.py:synth_inputs). Stored: the final four outputs (masks at every fourth query to stay under
1 MB), the class logits of all 10 prediction steps, a sub-sample of the masks of all steps, noise_* = max |fp32 - fp64| of the
reference's own outputs over all steps, and per layer the number of interpolated fp64 mask logits with |x| < tau = 8 * noise_masks.
No program text of the reference goes into the fixture.
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from multishiftseg_amd import synth  # noqa: E402
import ref_transformer_decoder as R  # noqa: E402

SEED, INPUT_SEED = 15, 151
SIZES, FEAT = [(3, 5), (6, 10), (12, 20)], (24, 40)
GEOM = dict(num_classes=19, hidden_dim=256, num_queries=100, nheads=8, dim_feedforward=2048, dec_layers=9, pre_norm=False,
            mask_dim=256, enforce_input_project=False)


def import_reference(ref):
    class Conv2d(torch.nn.Conv2d):                       # detectron2.layers.wrappers.Conv2d without norm / activation
        pass

    def c2_xavier_fill(module):                          # fvcore.nn.weight_init.c2_xavier_fill
        torch.nn.init.kaiming_uniform_(module.weight, a=1)
        if module.bias is not None:
            torch.nn.init.constant_(module.bias, 0)

    class Registry:                                      # detectron2.utils.registry.Registry: register() as a decorator
        def __init__(self, name):
            self.name = name

        def register(self, obj=None):
            return obj if obj is not None else (lambda c: c)

    stubs = {
        "fvcore": {}, "fvcore.nn": {}, "fvcore.nn.weight_init": {"c2_xavier_fill": c2_xavier_fill},
        "detectron2": {}, "detectron2.config": {"configurable": lambda f=None, **k: f if f is not None else (lambda g: g)},
        "detectron2.layers": {"Conv2d": Conv2d}, "detectron2.utils": {}, "detectron2.utils.registry": {"Registry": Registry},
    }
    for name, attrs in stubs.items():
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
    sys.modules["fvcore.nn"].weight_init = sys.modules["fvcore.nn.weight_init"]
    base = os.path.join(ref, "lib/network/mask2former/modeling")
    for name, sub in {"m2ftd": "", "m2ftd.transformer_decoder": "transformer_decoder"}.items():
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(base, sub)]
        sys.modules[name] = m
    return importlib.import_module("m2ftd.transformer_decoder.mask2former_transformer_decoder").MultiScaleMaskedTransformerDecoder_GMA


def run(Dec, sd, x, feat, dtype):
    """-> (outputs of every step, interpolated mask logits of every layer) of the reference in `dtype`."""
    dec = Dec(256, True, **GEOM).eval()
    dec.load_state_dict(sd, strict=True)
    dec = dec.to(dtype)
    steps, interp = [], []
    heads, ood = dec.forward_prediction_heads, dec.forward_ood_heads

    def pred(output, mask_features, attn_mask_target_size):
        r = heads(output, mask_features, attn_mask_target_size)
        steps.append([r[0], r[1]])
        interp.append(R.interp_logits(r[1], attn_mask_target_size))
        return r

    def pred_ood(output, mask_features, attn_mask_target_size):
        r = ood(output, mask_features, attn_mask_target_size)
        steps[-1] += [r[0], r[1]]
        return r
    dec.forward_prediction_heads, dec.forward_ood_heads = pred, pred_ood
    with torch.no_grad():
        out = dec([torch.from_numpy(v).to(dtype) for v in x], torch.from_numpy(feat).to(dtype))
    return out, steps, interp[:GEOM["dec_layers"]], list(dec.state_dict().items())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("MSS_REFERENCE"), help="checkout of the reference project (or MSS_REFERENCE)")
    args = ap.parse_args()
    if not args.reference:
        ap.error("give --reference DIR (or set MSS_REFERENCE): the reference project is not part of this repository")
    Dec = import_reference(args.reference)
    torch.manual_seed(0)
    names = list(Dec(256, True, **GEOM).state_dict().items())
    sd = {k: torch.from_numpy(synth.gen_tensor(SEED, "m2ftd." + k, tuple(v.shape), gain=1.0)) for k, v in names}
    x, feat = R.synth_inputs(INPUT_SEED, 2, SIZES, FEAT)
    o32, s32, i32, _ = run(Dec, sd, x, feat, torch.float32)
    o64, s64, i64, _ = run(Dec, sd, x, feat, torch.float64)
    n = lambda t: t.detach().cpu().numpy()
    dmax = lambda a, b: float((a.double() - b.double()).abs().max())
    noise_class = max(max(dmax(a[0], b[0]) for a, b in zip(s32, s64)), max(dmax(a[2], b[2]) for a, b in zip(s32[1:], s64[1:])))
    noise_masks = max(dmax(a[1], b[1]) for a, b in zip(s32, s64))
    tau = 8.0 * noise_masks
    near = np.array([int((t.abs() < tau).sum()) for t in i64], dtype=np.int64)
    flips = sum(int(((a < 0) != (b < 0)).sum() + ((a > 0) != (b > 0)).sum()) for a, b in zip(i32, i64))
    shapes = np.zeros((len(names), 4), dtype=np.int64)
    for j, (_, v) in enumerate(names):
        shapes[j, :v.dim()] = v.shape
    fix = {
        "seed": np.int64(SEED), "input_seed": np.int64(INPUT_SEED), "sizes": np.array(SIZES + [FEAT], dtype=np.int64),
        "names": np.array([k for k, _ in names]), "shapes": shapes, "ndim": np.array([v.dim() for _, v in names], dtype=np.int64),
        "pred_logits": n(o32["pred_logits"]), "pred_logits_ood": n(o32["pred_logits_ood"]),
        "pred_masks_q0of4": n(o32["pred_masks"][:, 0::4]), "pred_masks_ood_q1of4": n(o32["pred_masks_ood"][:, 1::4]),
        "n_aux": np.int64(len(o32["aux_outputs"])),
        "aux_last_logits": n(o32["aux_outputs"][-1]["pred_logits"]), "aux_last_logits_ood": n(o32["aux_outputs"][-1]["pred_logits_ood"]),
        "all_logits": np.stack([n(s[0]) for s in s32]), "all_logits_ood": np.stack([n(s[2]) for s in s32[1:]]),
        "all_masks_sub": np.stack([n(s[1][:, ::10, ::2, ::2]) for s in s32]),
        "noise_class": np.float64(noise_class), "noise_masks": np.float64(noise_masks), "tau": np.float64(tau),
        "near_count": near, "mask_rms": np.float64(float(o64["pred_masks"].pow(2).mean().sqrt())),
        "class_rms": np.float64(float(o64["pred_logits"].pow(2).mean().sqrt())),
        "min_abs_interp": np.float64(min(float(t.abs().min()) for t in i64)), "ref_bit_flips_fp32_vs_fp64": np.int64(flips),
    }
    path = os.path.join(ROOT, "tests", "golden", "m2f_transformer_decoder.npz")
    np.savez_compressed(path, **fix)
    print(f"wrote {path}: {os.path.getsize(path)} bytes; noise class {noise_class:.3g} masks {noise_masks:.3g} tau {tau:.3g} "
          f"near {near.tolist()} min|interp| {float(fix['min_abs_interp']):.3g} flips {flips} mask rms {float(fix['mask_rms']):.3g}")


if __name__ == "__main__":
    main()
