"""Build-time properties of k_bdx_fill (dpx_bdx_kernels.hip: band-direction batches under dpx_batch_set_direction_scoring) in the gfx950
code object, read from the code-object metadata on the CPU: the unit holds exactly the 48 instantiations (6 modes x 4 cells per lane x
2 parities) and nothing else, none uses scratch, every fill stays within 128 VGPRs at C = 1, 2, 4 and within 168 (three waves per
SIMD, the floor k_zsub_fill is held to) at C = 8, and no k_bdx kernel lives in dpx_banddir_kernels.  The counts are printed beside
k_bdir_fill's at the same C.  Metadata only: no instruction is looked at."""
import re

import pytest

import isa_units
from test_banddir_kernels_isa import BANNED

# (EXT, TABLE, SCAN): BANW takes a table only; BAXT every combination but none, which is k_bdir_fill
MODES = [(0, 1, 0), (1, 1, 0), (1, 0, 1), (1, 0, 2), (1, 1, 1), (1, 1, 2)]


@pytest.fixture(scope="module")
def units():
    names = ("dpx_bdx_kernels", "dpx_banddir_kernels")
    isa_units.text(*names)  # the two compile side by side
    return {u: {name: c[:2] for name, c in isa_units.counts(u).items()} for u in names}


def test_forty_eight_fills_nothing_else_and_no_scratch(units):
    meta = units["dpx_bdx_kernels"]
    assert len(meta) == 48 and all("k_bdx_fill" in k for k in meta), sorted(meta)
    for frag in {f"k_bdx_fillILi{c}ELb{pb}ELb{ext}ELb{tab}ELi{scan}EE" for c in (1, 2, 4, 8) for pb in (0, 1) for ext, tab, scan in MODES}:
        assert sum(frag in k for k in meta) == 1, frag
    for name, (vgprs, scratch) in meta.items():
        assert scratch == 0, (name, scratch)
        for banned in BANNED + ("k_bdir_fill", "k_zsub_fill"):  # substrings the other ISA tests count kernels by
            assert banned not in name, name
    assert not any("k_bdx" in k for k in units["dpx_banddir_kernels"])  # ... and the kernel lives in no other unit


def test_register_budget(units):
    bdx, bdir = {}, {}
    for name, (vgprs, _) in units["dpx_bdx_kernels"].items():
        c, ext, tab, scan = re.search(r"k_bdx_fillILi(\d)ELb[01]ELb([01])ELb([01])ELi([012])EE", name).groups()
        bdx.setdefault((int(c), int(ext), int(tab), int(scan)), []).append(vgprs)
    for name, (vgprs, _) in units["dpx_banddir_kernels"].items():
        m = re.search(r"k_bdir_fillILi(\d)ELb[01]ELb([01])EE", name)
        if m:
            bdir.setdefault((int(m.group(1)), int(m.group(2))), []).append(vgprs)
    for c in (1, 2, 4, 8):
        print(f"C={c}: k_bdir_fill BANW end {sorted(bdir[c, 0])}, BAXT end {sorted(bdir[c, 1])} vgprs; k_bdx_fill "
              + ", ".join(f"(EXT={e} TABLE={t} SCAN={s}) {sorted(bdx[c, e, t, s])}" for e, t, s in MODES))
        for mode in MODES:
            assert len(bdx[(c,) + mode]) == 2, (c, mode)
        worst = max(v for mode in MODES for v in bdx[(c,) + mode])
        assert worst <= (168 if c == 8 else 128), (c, worst)
