"""Build-time properties of the banded affine-gap extension fill (dpx_baxt_kernels.hip) in the gfx950 code object, read from the code-
object metadata on the CPU: all 16 instantiations of k_baxt_fill exist and nothing else lives in the unit, none uses scratch, and at
every cells-per-lane count C the register count allows at least as many waves per SIMD as k_basw_fill's of the same C."""
import re

import pytest

import isa_units



_waves_per_simd = isa_units.waves_per_simd


def _fills(meta, stem):
    """{C: [vgpr counts of the four instantiations]}"""
    out = {}
    for name, (vgprs, _) in meta.items():
        m = re.search(stem + r"ILi(\d)ELb[01]ELb[01]EE", name)
        if m:
            out.setdefault(int(m.group(1)), []).append(vgprs)
    return out


@pytest.fixture(scope="module")
def units():
    """{unit: {mangled name: (vgpr_count, private_segment_fixed_size)}} from the code object's kernel metadata"""
    names = ("dpx_baxt_kernels", "dpx_basw_kernels")
    isa_units.text(*names)  # the two compile side by side
    return {u: {name: c[:2] for name, c in isa_units.counts(u).items()} for u in names}


def test_sixteen_fills_and_no_scratch(units):
    meta = units["dpx_baxt_kernels"]
    assert len(meta) == 16 and all("k_baxt_fill" in k for k in meta), sorted(meta)
    for frag in {f"k_baxt_fillILi{c}ELb{pb}ELb{st}EE" for c in (1, 2, 4, 8) for pb in (0, 1) for st in (0, 1)}:
        assert sum(frag in k for k in meta) == 1, frag
    for name, (vgprs, scratch) in meta.items():
        assert scratch == 0, (name, scratch)
        # substrings the other ISA tests count kernels by
        for banned in ("k_basw", "k_banw", "k_asw_", "k_asg_", "k_banded_fill"):
            assert banned not in name, name


def test_occupancy_is_not_below_basw(units):
    baxt, basw = _fills(units["dpx_baxt_kernels"], "k_baxt_fill"), _fills(units["dpx_basw_kernels"], "k_basw_fill")
    assert sorted(baxt) == sorted(basw) == [1, 2, 4, 8] and all(len(v) == 4 for v in list(baxt.values()) + list(basw.values()))
    for c in (1, 2, 4, 8):
        print(f"C={c}: k_baxt_fill {sorted(baxt[c])} vgprs, k_basw_fill {sorted(basw[c])} vgprs")
        assert _waves_per_simd(max(baxt[c])) >= _waves_per_simd(max(basw[c])), (c, baxt[c], basw[c])
    assert _waves_per_simd(max(baxt[8])) >= 4
