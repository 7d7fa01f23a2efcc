"""DPX_ALGO_BAXT above the library: the Python constants, the header's enum value, and the C++ host mirror with its
BandedAffineExtension class and the drivers' -algo BAXT.  CPU only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "hostcpp")


def test_public_constants():
    import dpx_gpu_genomics_project_amd as dpx

    assert dpx.ALGO_BAXT == 10 and dpx.capi.ALGO_BAXT == 10
    assert dpx.ALGO_NAMES[10] == "BAXT" and "ALGO_BAXT" in dpx.__all__
    assert 8 not in dpx.ALGO_NAMES and 9 not in dpx.ALGO_NAMES
    header = open(os.path.join(ROOT, "include", "dpx_align.h")).read()
    assert re.search(r"\bDPX_ALGO_BAXT\s*=\s*10\b", header)
    assert "#define DPX_ABI_VERSION 3" in header
    kernels = open(os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "csrc", "dpx_kernels.h")).read()
    assert re.search(r"#define\s+DPX_K_BAXT\s+10\b", kernels) and "dpx_launch_baxt_fill" in kernels


def test_hostcpp_builds_with_the_new_class():
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    members = subprocess.run(["ar", "t", os.path.join(HOST, "libdpxhost.a")], check=True, capture_output=True, text=True).stdout.split()
    assert "BandedAffineExtension.o" in members, members
    for tool in ("dpx_main", "dpx_class_main"):
        r = subprocess.run([os.path.join(HOST, tool)], capture_output=True, text=True)
        assert "BAXT" in r.stderr, (tool, r.stderr)
