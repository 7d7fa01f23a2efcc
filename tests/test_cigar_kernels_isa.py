"""Build-time properties of the CIGAR kernels (dpx_cigar_kernels.hip) in the gfx950 code object, read from the code-object metadata on
the CPU: the unit compiles, every kernel in it is a k_cigar_* kernel whose name holds none of the substrings the other ISA tests
count kernels by, and none of them uses scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "csrc")
COUNTED_ELSEWHERE = ("k_basw", "k_banw", "k_baxt", "k_asw_", "k_asg_", "k_banded_fill", "k_linear_dir", "k_affine_dir", "k_traceback_wave")


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    """{mangled name: private_segment_fixed_size} from the code object's kernel metadata"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this machine")
    out = tmp_path_factory.mktemp("cigar_isa") / "dpx_cigar_kernels.s"
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I", CSRC, "-I",
                        os.path.join(ROOT, "include"), os.path.join(CSRC, "dpx_cigar_kernels.hip"), "-o", str(out)], capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    isa = open(out).read()
    found = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", isa, re.S):
        block = m.group(0)
        found[re.search(r"\.name:\s+(\S+)", block).group(1)] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
    return found


def test_the_unit_holds_the_three_stages(meta):
    for stage in ("k_cigar_count", "k_cigar_scan", "k_cigar_write"):
        assert any(stage in name for name in meta), (stage, sorted(meta))


def test_every_kernel_is_a_cigar_kernel(meta):
    for name in meta:
        assert re.search(r"\d+k_cigar_[a-z_]+", name), name  # (Itanium mangling: <length><identifier>)
        for banned in COUNTED_ELSEWHERE:
            assert banned not in name, (name, banned)


def test_no_kernel_uses_scratch(meta):
    for name, scratch in meta.items():
        assert scratch == 0, (name, scratch)
