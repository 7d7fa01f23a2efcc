"""Build-time properties of dpx_bscore_kernels.hip and dpx_lscore_kernels.hip (DPX_LONG_SCORES: the band-direction fills with nothing
stored but the results) in the gfx950 code object, on the CPU: the units hold exactly the 64 and the 32 fills and nothing else; no
kernel uses scratch or static LDS; every fill stays at or under the VGPR count of its storing twin (k_bdir_fill / k_bdx_fill / k_bdl_fill
/ k_bdlt_fill of the same parameters), counts printed; no fill body holds a 16-byte global store -- the storing twins put a code group
out with one, here the results and the extension record leave as dword stores, so "nothing but results leaves" reads off the store
mnemonics; no name carries a fragment another ISA test counts kernels by; and none of the kernels lives in another band-direction unit.
Metadata and isa_units.stores only."""
import re

import pytest

import isa_units
from test_banddir_kernels_isa import BANNED

NEW = ("dpx_bscore_kernels", "dpx_lscore_kernels")
TWINS = ("dpx_banddir_kernels", "dpx_bdx_kernels", "dpx_bdl_kernels", "dpx_bdlt_kernels")
OTHERS = TWINS + ("dpx_bd2_kernels", "dpx_lb2_kernels")
# BANW: (EXT = 0, SCAN = 0) with TABLE 0 / 1; BAXT: every (TABLE, SCAN)
BSCORE_MODES = [(0, t, 0) for t in (0, 1)] + [(1, t, s) for t in (0, 1) for s in (0, 1, 2)]
COUNTED_ELSEWHERE = BANNED + ("k_bdir", "k_bdx", "k_bd2", "k_bdl", "k_lb2", "k_zsub_fill")


@pytest.fixture(scope="module")
def units():
    isa_units.text(*(NEW + OTHERS))  # they compile side by side
    return {u: isa_units.kernels(u) for u in NEW + OTHERS}


def _one(kernels, fragment):
    hits = [k for k in kernels if fragment in k]
    assert len(hits) == 1, (fragment, hits)
    return hits[0]


def _pairs(units):
    """[(label, new kernel name, new unit, twin name, twin unit)] for all 96 fills"""
    out = []
    for c in (1, 2, 4, 8):
        for pb in (0, 1):
            for ext, table, scan in BSCORE_MODES:
                new = _one(units["dpx_bscore_kernels"], f"k_bscore_fillILi{c}ELb{pb}ELb{ext}ELb{table}ELi{scan}EE")
                if table or scan:
                    twin, unit = _one(units["dpx_bdx_kernels"], f"k_bdx_fillILi{c}ELb{pb}ELb{ext}ELb{table}ELi{scan}EE"), "dpx_bdx_kernels"
                else:
                    twin, unit = _one(units["dpx_banddir_kernels"], f"k_bdir_fillILi{c}ELb{pb}ELb{ext}EE"), "dpx_banddir_kernels"
                out.append((f"bscore C={c} PB={pb} EXT={ext} TABLE={table} SCAN={scan}", new, "dpx_bscore_kernels", twin, unit))
            for affine in (0, 1):
                for table in (0, 1):
                    new = _one(units["dpx_lscore_kernels"], f"k_lscore_fillILi{c}ELb{pb}ELb{affine}ELb{table}EE")
                    unit = "dpx_bdlt_kernels" if table else "dpx_bdl_kernels"
                    twin = _one(units[unit], f"k_bdl{'t' if table else ''}_fillILi{c}ELb{pb}ELb{affine}EE")
                    out.append((f"lscore C={c} PB={pb} AFFINE={affine} TABLE={table}", new, "dpx_lscore_kernels", twin, unit))
    return out


def test_exactly_the_fills_and_nothing_else(units):
    pairs = _pairs(units)
    assert len(pairs) == 96 and len({p[1] for p in pairs}) == 96
    assert sorted(units["dpx_bscore_kernels"]) == sorted(p[1] for p in pairs if p[2] == "dpx_bscore_kernels") and len(units["dpx_bscore_kernels"]) == 64
    assert sorted(units["dpx_lscore_kernels"]) == sorted(p[1] for p in pairs if p[2] == "dpx_lscore_kernels") and len(units["dpx_lscore_kernels"]) == 32
    for unit in NEW:
        for name in units[unit]:
            for counted in COUNTED_ELSEWHERE:
                assert counted not in name, (name, counted)
    for unit in OTHERS:
        assert not any("k_bscore" in k or "k_lscore" in k for k in units[unit]), unit


def test_no_scratch_no_static_lds_and_no_16_byte_store(units):
    for unit in NEW:
        for name, (meta, body, _) in units[unit].items():
            assert isa_units.field(meta, "private_segment_fixed_size") == 0, name
            assert isa_units.field(meta, "group_segment_fixed_size") == 0, name  # (the staged strings are dynamic LDS)
            stores = isa_units.stores(body)
            assert body and stores == {"global_store_dword"}, (name, stores)
    # what the assertion tells apart: every storing twin puts its code groups out with 16-byte stores
    for _, _, _, twin, unit in _pairs(units):
        assert "global_store_dwordx4" in isa_units.stores(units[unit][twin][1]), twin


def test_vgprs_at_or_under_the_storing_twin(units):
    over = []
    for label, new, unit, twin, twin_unit in _pairs(units):
        mine, theirs = isa_units.vgprs(units[unit][new][0]), isa_units.vgprs(units[twin_unit][twin][0])
        print(f"{label}: {mine} vgprs ({isa_units.waves_per_simd(mine)} waves per SIMD), storing twin {theirs} ({isa_units.waves_per_simd(theirs)})")
        if mine > theirs:
            over.append((label, mine, theirs))
    assert not over, over
