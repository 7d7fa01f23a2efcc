"""Build-time properties of the banded affine-gap Needleman-Wunsch kernels (dpx_banw_kernels.hip) in the gfx950 code object, checked on
the CPU: every instantiation of k_banw_fill, the export and both walks exist, none uses scratch or the matrix cores, the storing fills
write 16 bytes per lane, and the register counts are the recorded ones.  Adding the translation unit changed no other kernel: every
kernel the other translation units produced before (tests/golden/kernel_vgprs_before_banw.json, from the parent commit) is still there
with the same register count."""
import json
import os
import re

import pytest

import isa_units

# .vgpr_count as measured when the kernels were written: the largest of the four instantiations of each cells-per-lane count C (every C
# keeps four waves per SIMD, <= 128 registers), the export and the two walks
FILL_VGPRS = {1: 51, 2: 59, 4: 75, 8: 124}
OTHER_VGPRS = {"k_banw_export": 18, "k_banw_tracebackE": 50, "k_banw_traceback_wave": 225}


def _kernels(unit):
    """{mangled name: (metadata, body)}"""
    return {name: v[:2] for name, v in isa_units.kernels(unit).items()}


_vgprs = isa_units.vgprs


@pytest.fixture(scope="module")
def banw_isa():
    return _kernels("dpx_banw_kernels")


def test_every_kernel_exists_without_scratch_or_mfma(banw_isa):
    fills = {k: v for k, v in banw_isa.items() if "k_banw_fill" in k}
    assert len(fills) == 16, sorted(fills)
    for frag in {f"k_banw_fillILi{c}ELb{pb}ELb{st}EE" for c in (1, 2, 4, 8) for pb in (0, 1) for st in (0, 1)}:
        assert sum(frag in k for k in fills) == 1, frag
    for frag in OTHER_VGPRS:
        assert sum(frag in k for k in banw_isa) == 1, (frag, sorted(banw_isa))
    assert len(banw_isa) == 19, sorted(banw_isa)
    for name, (meta, body) in banw_isa.items():
        assert body, name
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), name
        assert "scratch_" not in body, name
        assert "v_mfma" not in body, name
        # substrings the other ISA tests count kernels by
        for banned in ("k_basw", "k_asw_", "k_asg_", "k_banded_fill", "k_linear_dir", "k_affine_dir", "k_traceback_waveILi3E"):
            assert banned not in name, name


def test_storing_fills_write_16_bytes_per_lane(banw_isa):
    for name, (meta, body) in banw_isa.items():
        if "k_banw_fill" not in name:
            continue
        stores = isa_units.stores(body)
        if name.endswith("ELb1EEEv13dpx_fill_args"):  # STORE = true: matrix stores are dwordx4 only (+ the three result dwords)
            assert "global_store_dwordx4" in stores, (name, stores)
            assert stores <= {"global_store_dwordx4", "global_store_dword"}, (name, stores)
        else:
            assert stores <= {"global_store_dword"}, (name, stores)


def test_register_counts_are_the_recorded_ones(banw_isa):
    seen = {}
    for name, (meta, body) in banw_isa.items():
        m = re.search(r"k_banw_fillILi(\d)E", name)
        if m:
            c = int(m.group(1))
            assert _vgprs(meta) <= FILL_VGPRS[c], (name, _vgprs(meta))
            seen[c] = max(seen.get(c, 0), _vgprs(meta))
        else:
            frag = [f for f in OTHER_VGPRS if f in name]
            assert len(frag) == 1 and _vgprs(meta) <= OTHER_VGPRS[frag[0]], (name, _vgprs(meta))
    assert sorted(seen) == [1, 2, 4, 8]
    assert all(seen[c] <= 128 for c in seen), seen  # four waves per SIMD at every C


def test_every_earlier_kernel_is_unchanged():
    golden = json.load(open(os.path.join(isa_units.ROOT, "tests", "golden", "kernel_vgprs_before_banw.json")))["kernels"]
    assert sorted(golden) == ["dpx_basw_kernels.hip", "dpx_dir_kernels.hip", "dpx_kernels.hip"]
    isa_units.text(*golden)  # they compile side by side
    for unit, want in golden.items():  # "dpx_kernels.hip": the union of the units it became (isa_units.SUCCESSORS), no name in two of them
        got = {k: _vgprs(v[0]) for k, v in _kernels(unit).items()}
        assert len(want) >= 19, unit
        assert got == want, (unit, sorted(set(got.items()) ^ set(want.items())))
        assert not [k for k in got if "banw" in k], unit  # the new kernels live in their own translation unit
