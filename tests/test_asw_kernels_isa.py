"""Build-time properties of the affine-gap Smith-Waterman kernels (k_asw_fill, k_asw_lanes, k_asw_dir, k_asw_traceback,
k_traceback_wave<3, false, ASW>) in the
gfx950 code object, checked on the CPU: no scratch, no matrix cores, the instructions of the ANW fill they share their body with, and a
register count that keeps four waves per SIMD."""
import re

import pytest

import isa_units



@pytest.fixture(scope="module")
def isa():
    return isa_units.kernels("dpx_kernels", "dpx_dir_kernels")


def _asw_kernels(isa):
    """{mangled name: (metadata, body)} of the kernels that run ASW"""
    return {name: v[:2] for name, v in isa.items() if "k_asw_" in name or "k_traceback_waveILi3ELb0ELi4E" in name}


_vgprs = isa_units.vgprs


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
        stores = isa_units.stores(body)
        assert stores and stores <= wide, (name, stores)
        assert "global_store_dwordx4" in stores, name
