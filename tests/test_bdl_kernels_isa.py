"""Build-time properties of dpx_bdl_kernels.hip (local band-direction batches of BSW / BASW) in the gfx950 code object, read from the
code-object metadata on the CPU: the unit holds exactly the 16 fills (4 cells-per-lane classes x 2 parities x linear / affine), one walk
and one export; no kernel of it uses scratch; every fill stays within 128 VGPRs (four waves per SIMD, the bound k_bdir_fill is held to);
the walk's LDS is the 16-KiB ring; no name carries a fragment another ISA test counts kernels by; and none of the kernels lives in
another band-direction unit.  The counts are printed.  Metadata only: no instruction is looked at."""
import re

import pytest

import isa_units
from test_banddir_kernels_isa import BANNED

OTHERS = ("dpx_banddir_kernels", "dpx_bdx_kernels", "dpx_bd2_kernels")


@pytest.fixture(scope="module")
def units():
    names = ("dpx_bdl_kernels",) + OTHERS
    isa_units.text(*names)  # they compile side by side
    return {u: isa_units.counts(u) for u in names}


def test_sixteen_fills_a_walk_an_export_and_no_scratch(units):
    meta = units["dpx_bdl_kernels"]
    fills = {k: v for k, v in meta.items() if "k_bdl_fill" in k}
    assert len(fills) == 16, sorted(meta)
    for frag in {f"k_bdl_fillILi{c}ELb{pb}ELb{affine}EE" for c in (1, 2, 4, 8) for pb in (0, 1) for affine in (0, 1)}:
        assert sum(frag in k for k in fills) == 1, frag
    others = sorted(k for k in meta if k not in fills)
    assert len(others) == 2 and "k_bdl_export" in others[0] and "k_bdl_traceback" in others[1], others
    for name, (vgprs, scratch, lds) in meta.items():
        assert scratch == 0, (name, scratch)
        for banned in BANNED + ("k_bdir_fill", "k_bdir", "k_bdx", "k_bd2", "k_zsub_fill"):
            assert banned not in name, name
    for unit in OTHERS:
        assert not any("k_bdl" in k for k in units[unit]), unit


def test_budget(units):
    meta = units["dpx_bdl_kernels"]
    by = {}
    for name, (vgprs, _, lds) in meta.items():
        m = re.search(r"k_bdl_fillILi(\d)ELb[01]ELb([01])EE", name)
        if m:
            by.setdefault((int(m.group(1)), int(m.group(2))), []).append(vgprs)
            assert lds == 0, (name, lds)  # (the staged strings are dynamic LDS)
    for (c, affine), counts in sorted(by.items()):
        print(f"C={c} {'BASW' if affine else 'BSW'}: k_bdl_fill {sorted(counts)} vgprs ({isa_units.waves_per_simd(max(counts))} waves per SIMD)")
        assert len(counts) == 2 and max(counts) <= 128, (c, affine, counts)
    walk = next(v for k, v in meta.items() if "k_bdl_traceback" in k)
    print(f"k_bdl_traceback {walk[0]} vgprs, {walk[2]} bytes of LDS")
    assert walk[2] == 16 * 1024, walk  # the ring of sixteen 1-KiB chunks
