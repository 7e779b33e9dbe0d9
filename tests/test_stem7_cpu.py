"""CPU: what hipcc makes of the 7x7 stem kernel (csrc/stem7.hip) for gfx950 -- its own kernel-resource-usage remarks and the assembly
text. The kernel keeps 49 weight registers per lane for the life of a workgroup; a spill would put loads in its tap loop."""
import os
import re
import subprocess

from conftest import ROOT


def test_stem7_kernel_uses_no_scratch_and_one_mfma_per_tap(tmp_path):
    src = os.path.join(ROOT, "multishiftseg_amd", "csrc", "stem7.hip")
    out = tmp_path / "stem7.s"
    r = subprocess.run(["hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "--cuda-device-only", "-S", src, "-o", str(out),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, cwd=os.path.dirname(src))
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(re.findall(r"Function Name: (\S+)", r.stderr)) == 1 and "stem7_conv_kernel" in r.stderr
    usage = {}
    for key in ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"):
        m = re.search(r" " + re.escape(key) + r": (\d+)", r.stderr)
        assert m, key
        usage[key] = int(m.group(1))
    assert usage["ScratchSize [bytes/lane]"] == 0 and usage["VGPRs Spill"] == 0 and usage["SGPRs Spill"] == 0, usage
    assert usage["VGPRs"] + usage["AGPRs"] <= 128 and usage["Occupancy [waves/SIMD]"] >= 4, usage      # four workgroups per CU
    assert usage["LDS Size [bytes/block]"] == 21 * 2 * 35 * 16, usage                                  # the input patch and nothing else
    # 49 taps x four independent accumulators, fully unrolled: the weights can only then stay in registers
    assert len(re.findall(r"^\s*v_mfma_f32_16x16x4_?f32\b", out.read_text(), flags=re.M)) == 4 * 49
