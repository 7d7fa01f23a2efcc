"""The host-side dispatchers of csrc/dpx_device.hpp (dispatch_int, dispatch_fill), which every launcher goes through: a stand-alone
host program (tests/dispatch_check.cpp, no GPU call) checks that each listed R / C, parity and flag reaches the callable exactly once
with those constants, that a value off the list returns hipErrorInvalidValue without a call, and that the callable's error comes back."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dispatchers_reach_the_right_instantiation(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this machine")
    exe = tmp_path / "dispatch_check"
    subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "csrc"),
                    "-o", str(exe), os.path.join(ROOT, "tests", "dispatch_check.cpp")], check=True, timeout=300)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "dispatchers ok" in r.stdout, r.stdout + r.stderr
