"""Build-time properties of the affine-gap semi-global kernels (k_asg_fill, k_asg_lanes, k_asg_dir, k_asg_traceback,
k_traceback_wave<3, false, ASG>) in the gfx950 code object, checked on the CPU: every instantiation exists, none uses scratch or the matrix
cores, the storing fills move their neighbours with DPP and write 16 bytes per lane as their ANW twins do, and every kernel keeps four
waves per SIMD (<= 128 VGPRs)."""
import re

import pytest

import isa_units


# .vgpr_count as measured when the kernels were written: (template arguments) -> registers
FILL_VGPRS = {("2", "1"): 58, ("2", "0"): 48, ("4", "1"): 74, ("4", "0"): 59, ("8", "1"): 101, ("8", "0"): 83}   # k_asg_fill<R, STORE>
LANES_VGPRS = {("8", "1"): 101, ("8", "0"): 52}                                                                  # k_asg_lanes<R, STORE>
DIR_VGPRS = {("2", "1"): 54, ("2", "0"): 52, ("4", "1"): 62, ("4", "0"): 60, ("8", "1"): 91, ("8", "0"): 88}   # k_asg_dir<R, GLOBAL>
WALK_VGPRS = {"k_asg_traceback": 78, "k_traceback_waveILi3ELb0ELi6E": 107}


@pytest.fixture(scope="module")
def isa():
    return {name: v[:2] for name, v in isa_units.kernels("dpx_kernels", "dpx_dir_kernels").items()
            if "k_asg_" in name or "k_traceback_waveILi3ELb0ELi6E" in name}


_vgprs = isa_units.vgprs


def _one(ks, frag):
    hits = [k for k in ks if frag in k]
    assert len(hits) == 1, (frag, sorted(ks))
    return hits[0]


def test_every_instantiation_exists_without_scratch_or_mfma(isa):
    assert len([k for k in isa if "k_asg_fill" in k]) == 6 and len([k for k in isa if "k_asg_lanes" in k]) == 2, sorted(isa)
    assert len([k for k in isa if "k_asg_dir" in k]) == 6, sorted(isa)
    for key in FILL_VGPRS:
        _one(isa, "k_asg_fillILi%sELb%sEE" % key)
    for key in LANES_VGPRS:
        _one(isa, "k_asg_lanesILi%sELb%sEE" % key)
    for key in DIR_VGPRS:
        _one(isa, "k_asg_dirILi%sELb%sEE" % key)
    for frag in WALK_VGPRS:
        _one(isa, frag)
    for name, (meta, body) in isa.items():
        assert body, name
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), name
        assert "scratch_" not in body, name
        assert "v_mfma" not in body, name
        # substrings the other ISA tests count kernels by
        for banned in ("k_asw_", "k_linear_dir", "k_affine_dir", "k_basw", "k_banded_fill", "k_traceback_waveILi3ELb0ELi4E"):
            assert banned not in name, name


def test_storing_fills_use_dpp_and_16_byte_stores(isa):
    for frag in ["k_asg_fillILi%sELb1EE" % r for r in "248"] + ["k_asg_lanesILi8ELb1EE"]:
        meta, body = isa[_one(isa, frag)]
        assert "v_mov_b32_dpp" in body, frag
        assert "v_max3_i32" in body, frag  # the shared recurrence
        stores = isa_units.stores(body)
        if "ILi8E" in frag:  # 8 rows per lane: one 16-byte piece per plane
            assert "global_store_dwordx4" in stores, (frag, stores)
    for frag in ["k_asg_fillILi%sELb0EE" % r for r in "248"] + ["k_asg_lanesILi8ELb0EE"]:  # score-only: the three result dwords alone
        meta, body = isa[_one(isa, frag)]
        assert "v_mov_b32_dpp" in body, frag
        assert isa_units.stores(body) <= {"global_store_dword"}, frag
    wide = {"global_store_dword", "global_store_dwordx2", "global_store_dwordx3", "global_store_dwordx4"}
    for key in DIR_VGPRS:
        meta, body = isa[_one(isa, "k_asg_dirILi%sELb%sEE" % key)]
        stores = isa_units.stores(body)
        assert stores and stores <= wide and "global_store_dwordx4" in stores, (key, stores)


def test_register_counts_keep_four_waves_per_simd(isa):
    got = {}
    for table, frag in ((FILL_VGPRS, "k_asg_fillILi%sELb%sEE"), (LANES_VGPRS, "k_asg_lanesILi%sELb%sEE"), (DIR_VGPRS, "k_asg_dirILi%sELb%sEE")):
        for key, recorded in table.items():
            name = _one(isa, frag % key)
            got[name] = _vgprs(isa[name][0])
            assert got[name] <= 128, (name, got[name])
            assert got[name] <= recorded, (name, got[name], recorded)
    for frag, recorded in WALK_VGPRS.items():
        name = _one(isa, frag)
        assert _vgprs(isa[name][0]) <= min(recorded, 128), (name, _vgprs(isa[name][0]))
