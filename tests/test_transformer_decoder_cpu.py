"""CPU: the stock-torch restatement of the GMA transformer decoder (tests/ref_transformer_decoder.py) reproduces the reference's
own outputs stored in tests/golden/m2f_transformer_decoder.npz, so that it can stand in for a reference that does not travel to
the GPU machine; and the HIP module keeps the reference's state_dict and refuses what it does not implement."""
import numpy as np
import pytest
import torch

import ref_transformer_decoder as R
from conftest import golden

GEOM = dict(num_classes=19, hidden_dim=256, num_queries=100, nheads=8, dim_feedforward=2048, dec_layers=9, pre_norm=False,
            mask_dim=256, enforce_input_project=False)


@pytest.fixture(scope="module")
def fix():
    return golden("m2f_transformer_decoder")


def _run(fix, dtype):
    sizes = [tuple(int(v) for v in s) for s in fix["sizes"]]
    x, feat = R.synth_inputs(int(fix["input_seed"]), 2, sizes[:3], sizes[3])
    sd = R.synth_state_dict(int(fix["seed"]), dtype=dtype)
    with torch.no_grad():
        return R.decoder_forward(sd, [torch.from_numpy(v).to(dtype) for v in x], torch.from_numpy(feat).to(dtype), 9, return_interp=True)


def _err(a, b):
    return float(np.abs(a.detach().double().numpy() - np.asarray(b, dtype=np.float64)).max())


@pytest.mark.parametrize("dtype,factor", [(torch.float32, 4.0), (torch.float64, 2.0)])
def test_helper_reproduces_the_reference_fixture(fix, dtype, factor):
    """Within 4 x noise of the stored fp32 outputs when run in fp32, within 2 x noise in fp64 (noise_* = max |fp32 - fp64| of the
    reference itself): final four outputs, the class logits of all 10 steps, the sub-sampled masks of all 10 steps, and the
    reference's off-by-one pairing of the auxiliary OOD outputs."""
    out = _run(fix, dtype)
    nc, nm = float(fix["noise_class"]), float(fix["noise_masks"])
    errs = {
        "pred_logits": (_err(out["pred_logits"], fix["pred_logits"]), nc),
        "pred_logits_ood": (_err(out["pred_logits_ood"], fix["pred_logits_ood"]), nc),
        "pred_masks": (_err(out["pred_masks"][:, 0::4], fix["pred_masks_q0of4"]), nm),
        "pred_masks_ood": (_err(out["pred_masks_ood"][:, 1::4], fix["pred_masks_ood_q1of4"]), nm),
        "all_logits": (_err(torch.stack(out["all_logits"]), fix["all_logits"]), nc),
        "all_logits_ood": (_err(torch.stack(out["all_logits_ood"][1:]), fix["all_logits_ood"]), nc),
        "all_masks": (_err(torch.stack([m[:, ::10, ::2, ::2] for m in out["all_masks"]]), fix["all_masks_sub"]), nm),
        "aux_last_logits": (_err(out["aux_outputs"][-1]["pred_logits"], fix["aux_last_logits"]), nc),
        "aux_last_logits_ood": (_err(out["aux_outputs"][-1]["pred_logits_ood"], fix["aux_last_logits_ood"]), nc),
    }
    print({k: (f"{e:.3g}", f"{factor * n:.3g}") for k, (e, n) in errs.items()})
    assert len(out["aux_outputs"]) == int(fix["n_aux"]) == 8
    bad = {k: (e, factor * n) for k, (e, n) in errs.items() if not e <= factor * n}
    assert not bad, bad


def test_fixture_thresholds_are_away_from_rounding(fix):
    """What the whole-decoder GPU test leans on: tau = 8 x noise_masks, the per-layer counts of near-zero interpolated logits are the
    helper's own in fp64, and the reference flips none of its mask bits between fp32 and fp64 on this geometry."""
    out = _run(fix, torch.float64)
    tau = float(fix["tau"])
    assert tau == 8.0 * float(fix["noise_masks"])
    assert [int((t.abs() < tau).sum()) for t in out["interp"]] == fix["near_count"].tolist()
    assert int(fix["ref_bit_flips_fp32_vs_fp64"]) == 0
    o32 = _run(fix, torch.float32)
    for (f64, b64), (f32, b32) in zip(out["bits"], o32["bits"]):
        assert torch.equal(f64, f32) and torch.equal(b64, b32)


def test_state_dict_matches_the_reference(fix):
    from multishiftseg_amd import MultiScaleMaskedTransformerDecoder_GMA
    with torch.device("meta"):
        m = MultiScaleMaskedTransformerDecoder_GMA(256, True, **GEOM)
    sd = m.state_dict()
    assert list(sd.keys()) == fix["names"].tolist()
    for (k, v), shape, nd in zip(sd.items(), fix["shapes"], fix["ndim"]):
        assert tuple(v.shape) == tuple(int(s) for s in shape[:int(nd)]), k
    assert {k: tuple(s) for k, s in R.param_shapes().items()} == {k: tuple(v.shape) for k, v in sd.items()}
    m2 = MultiScaleMaskedTransformerDecoder_GMA(256, True, **GEOM)
    m2.load_state_dict(R.synth_state_dict(int(fix["seed"])), strict=True)


@pytest.mark.parametrize("change", [dict(pre_norm=True), dict(hidden_dim=128), dict(nheads=4), dict(num_queries=129), dict(mask_dim=200)])
def test_unsupported_configuration_raises(change):
    from multishiftseg_amd import MultiScaleMaskedTransformerDecoder_GMA
    with pytest.raises(NotImplementedError):
        MultiScaleMaskedTransformerDecoder_GMA(256, True, **dict(GEOM, **change))


def test_cpu_forward_raises():
    from multishiftseg_amd import MultiScaleMaskedTransformerDecoder_GMA
    m = MultiScaleMaskedTransformerDecoder_GMA(256, True, **dict(GEOM, dec_layers=1))
    x = [torch.zeros(1, 256, h, w) for h, w in ((3, 5), (6, 10), (12, 20))]
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(x, torch.zeros(1, 256, 24, 40))


def test_workspace_query_is_host_only():
    from multishiftseg_amd import _lib
    assert _lib.value("mss_m2f_attn_workspace_bytes", 1, 100, 2, 128) == 1 * 2 * 8 * 128 * 34 * 128 * 4
    assert _lib.value("mss_m2f_attn_workspace_bytes", 2, 37, 1, 3) == 2 * 1 * 8 * 3 * 34 * 64 * 4
    assert _lib.value("mss_m2f_attn_workspace_bytes", 1, 100, 2, 1) == 0 and _lib.value("mss_m2f_attn_workspace_bytes", 1, 129, 2, 4) == 0
