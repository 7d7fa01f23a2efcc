"""Build-time properties of BAXT's extension-mode fill (dpx_zext_kernels.hip) in the gfx950 code object, read from the code-object
metadata on the CPU: all 32 instantiations of k_zext_fill exist and nothing else lives in the unit, none uses scratch, and at every
cells-per-lane count C the register count allows at least 4 waves per SIMD, the floor the project sets for k_baxt_fill at C = 8."""
import re

import pytest

import isa_units



_waves_per_simd = isa_units.waves_per_simd


@pytest.fixture(scope="module")
def units():
    """{unit: {mangled name: (vgpr_count, private_segment_fixed_size)}} from the code object's kernel metadata"""
    names = ("dpx_zext_kernels", "dpx_baxt_kernels")
    isa_units.text(*names)  # the two compile side by side
    return {u: {name: c[:2] for name, c in isa_units.counts(u).items()} for u in names}


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
