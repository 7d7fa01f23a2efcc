"""DPX_ALGO_BANW above the library: the Python constants, the header's enum value, and the C++ host mirror with its
BandedAffineNeedlemanWunsch class and the drivers' -algo BANW.  CPU only."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "hostcpp")


def test_public_constants():
    import dpx_gpu_genomics_project_amd as dpx

    assert dpx.ALGO_BANW == 7 and dpx.capi.ALGO_BANW == 7
    assert dpx.ALGO_NAMES[7] == "BANW" and "ALGO_BANW" in dpx.__all__
    header = open(os.path.join(ROOT, "include", "dpx_align.h")).read()
    assert re.search(r"\bDPX_ALGO_BANW\s*=\s*7\b", header)
    assert "#define DPX_ABI_VERSION 3" in header


def test_hostcpp_builds_with_the_new_class():
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    members = subprocess.run(["ar", "t", os.path.join(HOST, "libdpxhost.a")], check=True, capture_output=True, text=True).stdout.split()
    assert "BandedAffineNeedlemanWunsch.o" in members, members
    for tool in ("dpx_main", "dpx_class_main"):
        r = subprocess.run([os.path.join(HOST, tool)], capture_output=True, text=True)
        assert "BANW" in r.stderr, (tool, r.stderr)
