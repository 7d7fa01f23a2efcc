"""The five BANW-family translation units (dpx_banw / dpx_baxt / dpx_zext / dpx_subst / dpx_banddir _kernels.hip) after they came to share
dpx_band_affine.hpp, against tests/golden/kernel_vgprs_before_band_sharing.json (mangled name -> .vgpr_count, from the commit before):
every unit still holds exactly the kernels it held, none uses scratch, and no kernel runs fewer waves per SIMD than it did.  Metadata
only: no instruction is looked at."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "csrc")


def _waves_per_simd(vgprs):
    """512 VGPRs per SIMD lane, allocated in blocks of 8, at most 8 waves"""
    return min(8, 512 // ((vgprs + 7) // 8 * 8))


def _metadata(isa):
    """{mangled name: (vgpr_count, private_segment_fixed_size)} from the code object's kernel metadata"""
    out = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", isa, re.S):
        block = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1)), int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)))
    return out


def test_same_kernels_no_scratch_and_no_fewer_waves_per_simd(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this machine")
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "kernel_vgprs_before_band_sharing.json")))["kernels"]
    assert sorted(golden) == ["dpx_banddir_kernels.hip", "dpx_banw_kernels.hip", "dpx_baxt_kernels.hip", "dpx_subst_kernels.hip", "dpx_zext_kernels.hip"]
    tmp = tmp_path_factory.mktemp("band_sharing")
    jobs = {}
    for unit in golden:  # the five compile side by side
        out = tmp / (unit[:-4] + ".s")
        jobs[unit] = (out, subprocess.Popen([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I", CSRC, "-I",
                                             os.path.join(ROOT, "include"), os.path.join(CSRC, unit), "-o", str(out)]))
    for unit, want in golden.items():
        out, proc = jobs[unit]
        assert proc.wait(timeout=900) == 0, unit
        got = _metadata(open(out).read())
        assert sorted(got) == sorted(want), (unit, sorted(set(got) ^ set(want)))
        for name, (vgprs, scratch) in got.items():
            print(f"{unit} {name}: {want[name]} -> {vgprs} vgprs")
            assert scratch == 0, (unit, name, scratch)
            assert _waves_per_simd(vgprs) >= _waves_per_simd(want[name]), (unit, name, want[name], vgprs)
