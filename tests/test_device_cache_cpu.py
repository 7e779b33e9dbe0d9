"""The per-device once-cache behind every launcher's device questions (csrc/mss_device.h, DESIGN "per-device state") on the host: a
stand-alone program (tests/device_cache_check.cpp, its own main) drives the cache with a fake probe from 8 threads over 16 devices and
checks that the probe ran once per device, that no reader saw a half-filled record, that a failed probe is returned and not cached,
and that indices -1 and 16 are refused. Built and run once with the host compiler's address and undefined-behaviour sanitizers and
once with its thread sanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "multishiftseg_amd", "csrc")


@pytest.mark.parametrize("sanitizers", ["address,undefined", "thread"])
def test_device_cache_under_sanitizers(tmp_path, sanitizers):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "device_cache_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-pthread", "-fsanitize=" + sanitizers, "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "device_cache_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", r.stdout + r.stderr
