"""Build-time properties of BAXT's extension-mode fill (dpx_zext_kernels.hip) in the gfx950 code object, read from the code-object
metadata on the CPU: all 32 instantiations of k_zext_fill exist and nothing else lives in the unit, none uses scratch, and at every
cells-per-lane count C the register count allows at least 4 waves per SIMD, the floor the project sets for k_baxt_fill at C = 8."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "csrc")


def _start(tmp, name):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this machine")
    out = tmp / (name + ".s")
    return out, subprocess.Popen([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I", CSRC, "-I",
                                  os.path.join(ROOT, "include"), os.path.join(CSRC, name + ".hip"), "-o", str(out)])


def _finish(job):
    out, proc = job
    assert proc.wait(timeout=900) == 0, out
    return open(out).read()


def _metadata(isa):
    """{mangled name: (vgpr_count, private_segment_fixed_size)} from the code object's kernel metadata"""
    out = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", isa, re.S):
        block = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = (int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1)), int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)))
    return out


def _waves_per_simd(vgprs):
    """gfx950: 512 registers per lane and SIMD, allocated in blocks of 8, at most 8 waves"""
    return min(8, 512 // ((vgprs + 7) // 8 * 8))


@pytest.fixture(scope="module")
def units(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("zext_isa")
    jobs = {u: _start(tmp, u) for u in ("dpx_zext_kernels", "dpx_baxt_kernels")}  # the two compile side by side
    return {u: _metadata(_finish(j)) for u, j in jobs.items()}


def test_thirty_two_fills_and_no_scratch(units):
    meta = units["dpx_zext_kernels"]
    assert len(meta) == 32 and all("k_zext_fill" in k for k in meta), sorted(meta)
    for frag in {f"k_zext_fillILi{c}ELb{pb}ELb{st}ELb{zd}EE" for c in (1, 2, 4, 8) for pb in (0, 1) for st in (0, 1) for zd in (0, 1)}:
        assert sum(frag in k for k in meta) == 1, frag
    for name, (vgprs, scratch) in meta.items():
        assert scratch == 0, (name, scratch)
        # substrings the other ISA tests count kernels by
        for banned in ("k_basw", "k_banw", "k_baxt", "k_asw_", "k_asg_", "k_banded_fill", "k_cigar"):
            assert banned not in name, name


def test_four_waves_per_simd_at_every_c(units):
    zext, baxt = {}, {}
    for name, (vgprs, _) in units["dpx_zext_kernels"].items():
        c, zd = re.search(r"k_zext_fillILi(\d)ELb[01]ELb[01]ELb([01])EE", name).groups()
        zext.setdefault((int(c), int(zd)), []).append(vgprs)
    for name, (vgprs, _) in units["dpx_baxt_kernels"].items():
        baxt.setdefault(int(re.search(r"k_baxt_fillILi(\d)ELb[01]ELb[01]EE", name).group(1)), []).append(vgprs)
    for c in (1, 2, 4, 8):
        print(f"C={c}: k_zext_fill without the drop test {sorted(zext[c, 0])}, with it {sorted(zext[c, 1])} vgprs; k_baxt_fill {sorted(baxt[c])} vgprs")
        assert len(zext[c, 0]) == len(zext[c, 1]) == 4
        assert _waves_per_simd(max(zext[c, 0] + zext[c, 1])) >= 4, (c, zext[c, 0], zext[c, 1])
