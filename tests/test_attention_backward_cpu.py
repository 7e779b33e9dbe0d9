"""CPU: the host side of the masked attention's backward -- the workspace query, the "no CPU path" errors, and hipcc's own
kernel-resource-usage remarks for csrc/m2f_attn.hip (every training-forward and backward instantiation compiles without scratch)."""
import os
import re
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT


def test_backward_workspace_query_is_host_arithmetic():
    """D of every query [B][A][8][QS] + (more than one chunk) the chunks' partial dQ [B][A][8][chunks][32][QS], QS = Q rounded up to 64."""
    from multishiftseg_amd import _lib
    assert _lib.value("mss_m2f_attn_bwd_workspace_bytes", 1, 100, 2, 128) == 1 * 2 * 8 * 128 * (1 + 128 * 32) * 4
    assert _lib.value("mss_m2f_attn_bwd_workspace_bytes", 2, 37, 1, 3) == 2 * 1 * 8 * 64 * (1 + 3 * 32) * 4
    assert _lib.value("mss_m2f_attn_bwd_workspace_bytes", 2, 37, 1, 1) == 2 * 1 * 8 * 64 * 4
    assert _lib.value("mss_m2f_attn_bwd_workspace_bytes", 1, 129, 2, 4) == 0 and _lib.value("mss_m2f_attn_bwd_workspace_bytes", 1, 100, 2, 0) == 0


def test_masked_attention_has_no_cpu_path():
    import multishiftseg_amd
    from multishiftseg_amd import kernels as K
    q, k, v = torch.zeros(4, 256), torch.zeros(6, 256), torch.zeros(6, 256)
    with pytest.raises(RuntimeError, match="no CPU path"):
        multishiftseg_amd.masked_attention(q.requires_grad_(True), k, v, 2, 2, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.m2f_masked_attention_lse(q, k, v, 2, 2, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.m2f_masked_attention_backward(q, k, v, q, torch.zeros(2, 1, 8, 2), q, 2, 2, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        K.mask_logits(torch.zeros(1, 4, 16), K.Act(torch.zeros(1, 2, 2, 16)), 4)


def test_trainable_decoder_has_no_cpu_path():
    from multishiftseg_amd import MultiScaleMaskedTransformerDecoder_GMA
    m = MultiScaleMaskedTransformerDecoder_GMA(256, True, num_classes=19, hidden_dim=256, num_queries=8, nheads=8, dim_feedforward=128,
                                               dec_layers=1, pre_norm=False, mask_dim=256, enforce_input_project=False)
    assert m.set_trainable() is m
    x = [torch.zeros(1, 256, 2, 2) for _ in range(3)]
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(x, torch.zeros(1, 256, 4, 4))


def test_new_attention_kernels_use_no_scratch(tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc here")
    src = os.path.join(ROOT, "multishiftseg_amd", "csrc", "m2f_attn.hip")
    r = subprocess.run(["hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "--cuda-device-only", "-S", src,
                        "-o", str(tmp_path / "m2f_attn.s"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True,
                       cwd=os.path.dirname(src))
    assert r.returncode == 0, r.stderr[-2000:]
    scratch, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    # <MASKED, DIRECT, LSE> of the forward: the two training instantiations; <MASKED> of dK/dV; <MASKED, DIRECT> of dQ; delta; dQ merge
    new = [k for k in scratch if "m2f_attn_bwd_" in k or re.search(r"m2f_masked_attention_kernelILb[01]ELb1ELb1E", k)]
    assert len(new) == 2 + 2 + 4 + 1 + 1, sorted(scratch)
    assert len([k for k in scratch if "m2f_masked_attention_kernel" in k]) == 6
    bad = {k: v for k, v in scratch.items() if v != 0}
    assert not bad, bad
