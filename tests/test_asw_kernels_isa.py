"""Build-time properties of the affine-gap Smith-Waterman kernels (k_asw_fill, k_asw_lanes, k_asw_dir, k_asw_traceback,
k_traceback_wave<3, false, ASW>) in the
gfx950 code object, checked on the CPU: no scratch, no matrix cores, the instructions of the ANW fill they share their body with, and a
register count that keeps four waves per SIMD."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "csrc")


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this machine")
    out = tmp_path_factory.mktemp("asw_isa") / "dpx_kernels.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(CSRC, "dpx_kernels.hip"), "-o", str(out)], check=True, timeout=600)
    dout = tmp_path_factory.mktemp("asw_isa_dir") / "dpx_dir_kernels.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(CSRC, "dpx_dir_kernels.hip"), "-o", str(dout)], check=True, timeout=600)
    return open(out).read() + "\n" + open(dout).read()


def _asw_kernels(isa):
    """{mangled name: (metadata, body)} of the kernels that run ASW"""
    meta = {m.group(1): m.group(0) for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n){0,12}?.*\.vgpr_count:\s+\d+", isa)}
    out = {}
    for name in meta:
        if "k_asw_" not in name and "k_traceback_waveILi3ELb0ELi4E" not in name:
            continue
        start = isa.find("\n" + name + ":")
        end = isa.find(".Lfunc_end", start)
        out[name] = (meta[name], isa[start:end] if start >= 0 else "")
    return out


def _vgprs(meta):
    return int(re.search(r"\.vgpr_count:\s+(\d+)", meta).group(1))


def test_asw_kernels_exist_without_scratch_or_mfma(isa):
    ks = _asw_kernels(isa)
    fills = [k for k in ks if "k_asw_fill" in k]
    assert len(fills) == 6, sorted(ks)  # R = 2, 4, 8 x matrices / score-only
    assert len([k for k in ks if "k_asw_lanes" in k]) == 2 and len([k for k in ks if "k_asw_dir" in k]) == 6, sorted(ks)
    assert any("k_asw_traceback" in k for k in ks) and any("k_traceback_wave" in k for k in ks), sorted(ks)
    for name, (meta, body) in ks.items():
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), name
        assert "scratch_" not in body, name
        assert "v_mfma" not in body, name


def test_asw_fills_use_the_shared_recurrence_and_stay_at_four_waves(isa):
    ks = _asw_kernels(isa)
    for name, (meta, body) in ks.items():
        if "k_asw_fill" not in name and "k_asw_lanes" not in name and "k_asw_dir" not in name:
            continue
        if "k_asw_dir" not in name:  # (the direction fill compares the candidates for its codes instead)
            assert "v_max3_i32" in body, name
        assert _vgprs(meta) <= 128, (name, _vgprs(meta))
    for frag in ("k_asw_fillILi8ELb1EE", "k_asw_lanesILi8ELb1EE"):
        meta, body = next(v for k, v in ks.items() if frag in k)
        assert "global_store_dwordx4" in body, frag


def test_asw_direction_stores_are_dword_or_wider(isa):
    wide = {"global_store_dword", "global_store_dwordx2", "global_store_dwordx3", "global_store_dwordx4"}
    for name, (meta, body) in _asw_kernels(isa).items():
        if "k_asw_dir" not in name:
            continue
        stores = set(re.findall(r"\b(global_store_\w+|buffer_store_\w+|flat_store_\w+)", body))
        assert stores and stores <= wide, (name, stores)
        assert "global_store_dwordx4" in stores, name
