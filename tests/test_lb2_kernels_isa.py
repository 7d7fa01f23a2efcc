"""Build-time properties of dpx_lb2_kernels.hip (two-piece local band-direction batches of BASW) in the gfx950 code object, read from
the code-object metadata on the CPU: the unit holds exactly the 12 fills (3 cells-per-lane classes x 2 parities x table or not), one walk
and one export; no kernel of it uses scratch; the walk's LDS is the 16-KiB ring; every fill allows at least as many waves per SIMD as
its twin k_bd2_fill<C, PB, true, TABLE, 0> of the same build; no name carries a fragment another ISA test counts kernels by; and none of
the kernels lives in another band-direction unit.  The counts are printed.  Metadata only: no instruction is looked at."""
import re

import pytest

import isa_units
from test_banddir_kernels_isa import BANNED

OTHERS = ("dpx_banddir_kernels", "dpx_bdx_kernels", "dpx_bd2_kernels", "dpx_bdl_kernels", "dpx_bdlt_kernels")
COUNTED_ELSEWHERE = BANNED + ("k_bdl", "k_bdlt", "k_bd2", "k_bdir", "k_bdx", "k_zsub_fill")


@pytest.fixture(scope="module")
def units():
    names = ("dpx_lb2_kernels",) + OTHERS
    isa_units.text(*names)  # they compile side by side
    return {u: isa_units.counts(u) for u in names}


def test_twelve_fills_a_walk_an_export_and_no_scratch(units):
    meta = units["dpx_lb2_kernels"]
    fills = {k: v for k, v in meta.items() if "k_lb2_fill" in k}
    assert len(fills) == 12, sorted(meta)
    for frag in {f"k_lb2_fillILi{c}ELb{pb}ELb{tab}EE" for c in (1, 2, 4) for pb in (0, 1) for tab in (0, 1)}:
        assert sum(frag in k for k in fills) == 1, frag
    others = sorted(k for k in meta if k not in fills)
    assert len(others) == 2 and "k_lb2_export" in others[0] and "k_lb2_traceback" in others[1], others
    for name, (vgprs, scratch, lds) in meta.items():
        assert scratch == 0, (name, scratch)
        for counted in COUNTED_ELSEWHERE:
            assert counted not in name, (name, counted)
    for unit in OTHERS:
        assert not any("k_lb2" in k for k in units[unit]), unit
    walk = next(v for k, v in meta.items() if "k_lb2_traceback" in k)
    print(f"k_lb2_traceback {walk[0]} vgprs, {walk[2]} bytes of LDS")
    assert walk[2] == 16 * 1024, walk  # the ring of sixteen 1-KiB chunks


def test_waves_per_simd_against_the_two_piece_twin(units):
    twin = {}
    for name, (vgprs, _, _) in units["dpx_bd2_kernels"].items():
        m = re.search(r"k_bd2_fillILi(\d)ELb([01])ELb1ELb([01])ELi0EE", name)  # <C, PB, EXT = true, TABLE, SCAN = 0>
        if m:
            twin[tuple(int(x) for x in m.groups())] = vgprs
    assert len(twin) == 12, sorted(twin)
    seen = 0
    for name, (vgprs, _, lds) in sorted(units["dpx_lb2_kernels"].items()):
        m = re.search(r"k_lb2_fillILi(\d)ELb([01])ELb([01])EE", name)
        if not m:
            continue
        key = tuple(int(x) for x in m.groups())
        mine, theirs = isa_units.waves_per_simd(vgprs), isa_units.waves_per_simd(twin[key])
        print(f"C={key[0]} PB={key[1]} TABLE={key[2]}: k_lb2_fill {vgprs} vgprs ({mine} waves per SIMD), k_bd2_fill twin {twin[key]} vgprs ({theirs})")
        assert lds == 0, (name, lds)  # (the staged strings are dynamic LDS)
        assert mine >= theirs, (key, vgprs, twin[key])
        seen += 1
    assert seen == 12
