"""Build-time properties of k_zsub_fill (dpx_zsub_kernels.hip: BAXT's extension mode under a substitution table) in the gfx950 code
object, read from the code-object metadata on the CPU: the unit holds exactly the 32 instantiations (C x PB x STORE x ZDROP) and
nothing else, none uses scratch, and the register count allows at least 4 waves per SIMD at C = 1, 2, 4 and at least 3 (168 VGPRs) at
C = 8.  The counts are printed beside k_subst_fill<EXT> and k_zext_fill at the same C.  Metadata only: no instruction is looked at."""
import re

import pytest

import isa_units


@pytest.fixture(scope="module")
def units():
    """{unit: {mangled name: (vgpr_count, private_segment_fixed_size)}} from the code objects' kernel metadata"""
    names = ("dpx_zsub_kernels", "dpx_subst_kernels", "dpx_zext_kernels")
    isa_units.text(*names)  # the three compile side by side
    return {u: {name: c[:2] for name, c in isa_units.counts(u).items()} for u in names}


def test_thirty_two_fills_nothing_else_and_no_scratch(units):
    meta = units["dpx_zsub_kernels"]
    assert len(meta) == 32 and all("k_zsub_fill" in k for k in meta), sorted(meta)
    for frag in {f"k_zsub_fillILi{c}ELb{pb}ELb{st}ELb{zd}EE" for c in (1, 2, 4, 8) for pb in (0, 1) for st in (0, 1) for zd in (0, 1)}:
        assert sum(frag in k for k in meta) == 1, frag
    for name, (vgprs, scratch) in meta.items():
        assert scratch == 0, (name, scratch)
        # substrings the other ISA tests count kernels by
        for banned in ("k_basw", "k_banw", "k_baxt", "k_zext_fill", "k_subst", "k_asw_", "k_asg_", "k_banded_fill", "k_cigar"):
            assert banned not in name, name
    for unit in ("dpx_subst_kernels", "dpx_zext_kernels"):  # ... and the kernel lives in no other unit
        assert not any("k_zsub_fill" in k for k in units[unit]), unit


def test_waves_per_simd(units):
    zsub, subst, zext = {}, {}, {}
    for name, (vgprs, _) in units["dpx_zsub_kernels"].items():
        c, zd = re.search(r"k_zsub_fillILi(\d)ELb[01]ELb[01]ELb([01])EE", name).groups()
        zsub.setdefault((int(c), int(zd)), []).append(vgprs)
    for name, (vgprs, _) in units["dpx_subst_kernels"].items():
        m = re.search(r"k_subst_fillILi(\d)ELb[01]ELb[01]ELb1EE", name)
        if m:
            subst.setdefault(int(m.group(1)), []).append(vgprs)
    for name, (vgprs, _) in units["dpx_zext_kernels"].items():
        zext.setdefault(int(re.search(r"k_zext_fillILi(\d)ELb", name).group(1)), []).append(vgprs)
    for c in (1, 2, 4, 8):
        print(f"C={c}: k_zsub_fill without the drop test {sorted(zsub[c, 0])}, with it {sorted(zsub[c, 1])} vgprs; "
              f"k_subst_fill<EXT> {sorted(subst[c])}, k_zext_fill {sorted(zext[c])} vgprs")
        assert len(zsub[c, 0]) == len(zsub[c, 1]) == 4 and len(subst[c]) == 4 and len(zext[c]) == 8
        worst = max(zsub[c, 0] + zsub[c, 1])
        assert isa_units.waves_per_simd(worst) >= (3 if c == 8 else 4), (c, zsub[c, 0], zsub[c, 1])
        if c == 8:
            assert worst <= 168, worst
