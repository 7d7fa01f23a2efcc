"""Build-time properties of the banded affine-gap Smith-Waterman kernels (dpx_basw_kernels.hip) in the gfx950 code object, checked on
the CPU: every instantiation of k_basw_fill exists, none uses scratch or the matrix cores, the storing ones write 16 bytes per lane and
move their neighbours with DPP, and the register counts are the recorded ones.  Adding the translation unit changed no other kernel:
every kernel dpx_kernels.hip / dpx_dir_kernels.hip produced before (tests/golden/kernel_vgprs_before_basw.json) is still there with the
same register count."""
import json
import os
import re

import pytest

import isa_units

# .vgpr_count per cells-per-lane count C as measured when the kernel was written (the largest of the four instantiations of that C):
# C <= 4 keeps more than four waves per SIMD (<= 128 registers), C = 8 exactly four
VGPR_BOUND = {1: 46, 2: 54, 4: 75, 8: 122}


def _kernels(unit):
    """{mangled name: (metadata, body)}"""
    return {name: v[:2] for name, v in isa_units.kernels(unit).items()}


_vgprs = isa_units.vgprs


@pytest.fixture(scope="module")
def basw_isa():
    return _kernels("dpx_basw_kernels")


def test_every_instantiation_exists_without_scratch_or_mfma(basw_isa):
    fills = {k: v for k, v in basw_isa.items() if "k_basw_fill" in k}
    want = {f"k_basw_fillILi{c}ELb{pb}ELb{st}EE" for c in (1, 2, 4, 8) for pb in (0, 1) for st in (0, 1)}
    assert len(fills) == 16, sorted(fills)
    for frag in want:
        assert sum(frag in k for k in fills) == 1, frag
    assert any("k_basw_export" in k for k in basw_isa) and any("k_basw_tracebackE" in k for k in basw_isa), sorted(basw_isa)
    assert any("k_basw_traceback_wave" in k for k in basw_isa), sorted(basw_isa)
    for name, (meta, body) in basw_isa.items():
        assert body, name
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), name
        assert "scratch_" not in body, name
        assert "v_mfma" not in body, name
        for banned in ("k_asw_", "k_banded_fill", "k_traceback_waveILi3ELb0ELi4E"):  # substrings the other ISA tests count kernels by
            assert banned not in name, name


def test_storing_fills_write_16_bytes_per_lane_and_move_neighbours_with_dpp(basw_isa):
    for name, (meta, body) in basw_isa.items():
        if "k_basw_fill" not in name:
            continue
        assert "v_mov_b32_dpp" in body, name
        stores = isa_units.stores(body)
        if name.endswith("ELb1EEEv13dpx_fill_args"):  # STORE = true: matrix stores are dwordx4 only (+ the three result dwords)
            assert "global_store_dwordx4" in stores, (name, stores)
            assert stores <= {"global_store_dwordx4", "global_store_dword"}, (name, stores)
        else:
            assert stores <= {"global_store_dword"}, (name, stores)


def test_register_counts_are_the_recorded_ones(basw_isa):
    seen = {}
    for name, (meta, body) in basw_isa.items():
        m = re.search(r"k_basw_fillILi(\d)E", name)
        if not m:
            continue
        c = int(m.group(1))
        assert _vgprs(meta) <= VGPR_BOUND[c], (name, _vgprs(meta))
        seen[c] = max(seen.get(c, 0), _vgprs(meta))
    assert sorted(seen) == [1, 2, 4, 8]
    assert all(seen[c] <= 128 for c in seen), seen  # four waves per SIMD at every C


def test_every_earlier_kernel_is_unchanged():
    golden = json.load(open(os.path.join(isa_units.ROOT, "tests", "golden", "kernel_vgprs_before_basw.json")))["kernels"]
    for unit, want in golden.items():
        got = {k: _vgprs(v[0]) for k, v in _kernels(unit).items()}  # "dpx_kernels.hip": the union of the units it became
        assert len(want) > 20, unit
        for name, vg in want.items():
            assert got.get(name) == vg, (unit, name, vg, got.get(name))
        assert not [k for k in got if "basw" in k], unit  # the new kernels live in their own translation unit
