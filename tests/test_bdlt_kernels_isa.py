"""Build-time properties of dpx_bdlt_kernels.hip (local band-direction batches of BSW / BASW under a substitution table) in the gfx950
code object, read from the code-object metadata on the CPU: the unit holds exactly the 16 fills (4 cells-per-lane classes x 2 parities x
linear / affine) and nothing else; none uses scratch; static LDS is 0 (strings and the table image are dynamic LDS); no name carries a
fragment another ISA test counts kernels by; and no table fill allows fewer waves per SIMD than its plain twin in dpx_bdl_kernels.hip.
The counts are printed side by side.  Metadata only: no instruction is looked at."""
import re

import pytest

import isa_units
from test_banddir_kernels_isa import BANNED as BANDDIR_BANNED
from test_subst_kernels_isa import BANNED as SUBST_BANNED

FRAGMENTS = tuple(sorted(set(BANDDIR_BANNED + SUBST_BANNED + ("k_bdl_fill", "k_bdl_traceback", "k_bdl_export", "k_bdir", "k_bdx", "k_bd2", "k_zsub_fill",
                                                               "k_dirtab", "k_scoretab"))))


@pytest.fixture(scope="module")
def units():
    names = ("dpx_bdlt_kernels", "dpx_bdl_kernels")
    isa_units.text(*names)  # they compile side by side
    return {u: isa_units.counts(u) for u in names}


def _by_shape(meta, kernel):
    out = {}
    for name, entry in meta.items():
        m = re.search(kernel + r"ILi(\d)ELb([01])ELb([01])EE", name)
        if m:
            key = tuple(int(x) for x in m.groups())
            assert key not in out, name
            out[key] = entry
    return out


def test_sixteen_fills_and_nothing_else(units):
    meta = units["dpx_bdlt_kernels"]
    fills = _by_shape(meta, "k_bdlt_fill")
    assert len(meta) == 16 and len(fills) == 16, sorted(meta)
    assert set(fills) == {(c, pb, affine) for c in (1, 2, 4, 8) for pb in (0, 1) for affine in (0, 1)}
    for name, (vgprs, scratch, lds) in meta.items():
        assert scratch == 0, (name, scratch)
        assert lds == 0, (name, lds)
        for fragment in FRAGMENTS:
            assert fragment not in name, (name, fragment)
    assert not any("k_bdlt" in k for k in units["dpx_bdl_kernels"])


def test_registers_beside_the_plain_twins(units):
    table, plain = _by_shape(units["dpx_bdlt_kernels"], "k_bdlt_fill"), _by_shape(units["dpx_bdl_kernels"], "k_bdl_fill")
    assert set(table) == set(plain) and len(plain) == 16
    for key in sorted(table):
        c, pb, affine = key
        tv, pv = table[key][0], plain[key][0]
        tw, pw = isa_units.waves_per_simd(tv), isa_units.waves_per_simd(pv)
        print(f"C={c} PB={pb} {'BASW' if affine else 'BSW'}: k_bdlt_fill {tv} vgprs ({tw} waves per SIMD), k_bdl_fill {pv} vgprs ({pw} waves per SIMD)")
        assert tv <= 128, (key, tv)  # four waves per SIMD, the bound the plain fills are held to
        assert tw >= pw, (key, tv, pv)  # the table costs no residency
