"""Build-time properties of k_scoretab_fill / k_scoretab_lanes (dpx_scoretab_kernels.hip: ANW / ASW / ASG score-only batches under
dpx_batch_set_score_table) in the gfx950 code object, read from the code-object metadata on the CPU: the unit holds exactly the 12
instantiations (3 kinds x 3 rows per lane, one wave per pair; 3 kinds lane-packed) and nothing else, none uses scratch, no scoretab
kernel lives in dpx_affine_kernels, and every table kernel allows as many waves per SIMD as the plain score-only kernel of the same rows
per lane and kind.  The register counts are printed side by side.  Metadata only: no instruction is looked at."""
import re

import pytest

import isa_units

KINDS = {2: ("ANW", "k_affine_"), 4: ("ASW", "k_asw_"), 6: ("ASG", "k_asg_")}  # DPX_K_ANW / _ASW / _ASG: the KIND argument


@pytest.fixture(scope="module")
def units():
    names = ("dpx_scoretab_kernels", "dpx_affine_kernels")
    isa_units.text(*names)  # the two compile side by side
    return {u: {name: c[:2] for name, c in isa_units.counts(u).items()} for u in names}


def test_twelve_kernels_nothing_else_and_no_scratch(units):
    meta = units["dpx_scoretab_kernels"]
    assert len(meta) == 12 and all("k_scoretab_" in k for k in meta), sorted(meta)
    frags = {f"k_scoretab_fillILi{r}ELi{kind}EE" for r in (2, 4, 8) for kind in KINDS} | {f"k_scoretab_lanesILi{kind}EE" for kind in KINDS}
    for frag in frags:
        assert sum(frag in k for k in meta) == 1, frag
    for name, (vgprs, scratch) in meta.items():
        assert scratch == 0, (name, scratch)
        for banned in ("k_affine_", "k_asw_", "k_asg_", "k_linear", "k_dirtab", "k_subst", "k_zsub", "k_bdx"):  # substrings the other ISA tests count kernels by
            assert banned not in name, name
    assert not any("k_scoretab" in k for k in units["dpx_affine_kernels"])  # ... and the kernels live in no other unit
    assert len(units["dpx_affine_kernels"]) == 24  # (the plain unit keeps its 18 fills and 6 lane-packed kernels)


def test_the_table_costs_no_wave_of_occupancy(units):
    tab, plain = {}, {}
    for name, (vgprs, _) in units["dpx_scoretab_kernels"].items():
        m = re.search(r"k_scoretab_fillILi(\d)ELi(\d)EE", name)
        if m:
            tab["fill", int(m.group(1)), int(m.group(2))] = vgprs
        else:
            tab["lanes", 8, int(re.search(r"k_scoretab_lanesILi(\d)EE", name).group(1))] = vgprs
    for name, (vgprs, _) in units["dpx_affine_kernels"].items():
        for kind, (_, stem) in KINDS.items():
            m = re.search(stem + r"(fill|lanes)ILi(\d)ELb0EE", name)  # STORE = false: the score-only instantiation
            if m:
                plain[m.group(1), int(m.group(2)), kind] = vgprs
    assert sorted(tab) == sorted(plain) and len(tab) == 12, (sorted(tab), sorted(plain))
    for key in sorted(tab):
        shape, r, kind = key
        t, p = tab[key], plain[key]
        print(f"{KINDS[kind][0]} {shape} R={r}: plain {p} vgprs ({isa_units.waves_per_simd(p)} waves/SIMD), table {t} vgprs ({isa_units.waves_per_simd(t)} waves/SIMD)")
    for key in sorted(tab):
        assert isa_units.waves_per_simd(tab[key]) == isa_units.waves_per_simd(plain[key]), (key, tab[key], plain[key])
