"""CPU: the per-image instantiations of gemm_nt_kernel (csrc/gemm.hip, the product behind the Dropout2d channel compaction) and the
compaction kernels (csrc/chan_compact.hip) cross-compile for gfx950 without scratch and at the occupancy of their dense twins --
hipcc's own kernel-resource-usage remarks, as tests/test_abi_cpu.py reads them for the split-bf16 kernels."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "multishiftseg_amd", "csrc")


def _usage(src, tmp_path):
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc here")
    r = subprocess.run(["hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "--cuda-device-only", "-S",
                        os.path.join(CSRC, src), "-o", str(tmp_path / (src + ".s")), "-Rpass-analysis=kernel-resource-usage"],
                       capture_output=True, text=True, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        for key in ("VGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]"):
            m = re.search(re.escape(key) + r": (\d+)", line)
            if m and name and "AGPRs" not in line:
                usage[name][key] = int(m.group(1))
    return usage


def _one(usage, tag):
    hits = [v for k, v in usage.items() if tag in k]
    assert len(hits) == 1, (tag, sorted(usage))
    return hits[0]


def test_per_image_gemm_instantiations_use_no_scratch(tmp_path):
    """Template arguments in the mangled names: <AFFINE, VARIANT, BN, PERIMG>. The per-image kernels keep the residency of the dense
    kernels they replace (two workgroups per CU on the 256-wide tile, three on the 128-wide one)."""
    usage = _usage("gemm.hip", tmp_path)
    for bn, occ in ((256, 2), (128, 3)):
        new = _one(usage, f"gemm_nt_kernelILb0ELi3ELi{bn}ELb1EE")
        dense = _one(usage, f"gemm_nt_kernelILb0ELi3ELi{bn}ELb0EE")
        assert new["ScratchSize [bytes/lane]"] == 0 and new["VGPRs"] <= 256, new
        assert new["Occupancy [waves/SIMD]"] == dense["Occupancy [waves/SIMD]"] == occ, (new, dense)
    # the hot dense instantiations of the step stay without scratch too
    for tag in ("gemm_nt_kernelILb1ELi3ELi256ELb0EE", "gemm_nt_kernelILb0ELi3ELi256ELb0EE", "gemm_nt_kernelILb0ELi3ELi128ELb0EE"):
        assert _one(usage, tag)["ScratchSize [bytes/lane]"] == 0, tag


def test_compaction_kernels_use_no_scratch(tmp_path):
    usage = _usage("chan_compact.hip", tmp_path)
    assert len(usage) == 5, sorted(usage)
    for k, v in usage.items():
        assert v["ScratchSize [bytes/lane]"] == 0, (k, v)
        if "chan_compact_rows_kernel" in k:
            assert v["VGPRs"] <= 128 and v["Occupancy [waves/SIMD]"] >= 4, (k, v)       # four 32-KB workgroups per CU


def test_abi_version_and_struct_tail_agree():
    """MssConvArgs.k_steps / w_img_stride are appended at the END of the struct in the header and in the ctypes mirror."""
    from multishiftseg_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mss_hip.h")).read()
    assert int(re.search(r"#define MSS_ABI_VERSION (\d+)", hdr).group(1)) == _lib.MSS_ABI_VERSION
    body = hdr[hdr.index("typedef struct MssConvArgs {"):hdr.index("} MssConvArgs;")]
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names[-2:] == ["k_steps", "w_img_stride"] and [f[0] for f in _lib.MssConvArgs._fields_][-2:] == names[-2:]
