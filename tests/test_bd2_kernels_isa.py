"""Build-time properties of k_bd2_fill (dpx_bd2_kernels.hip: two-piece band-direction batches) in the gfx950 code object, read from the
code-object metadata on the CPU: the unit holds exactly the 48 fills (8 modes x 3 cells per lane x 2 parities) beside its walk and its
export, no kernel of it uses scratch, every fill stays within 128 VGPRs at C = 1, 2 and within 256 at C = 4 (C = 8 is not built: it
does not fit the register file), and no k_bd2 kernel lives in the one-piece units.  The counts are printed.  Metadata only: no
instruction is looked at."""
import re

import pytest

import isa_units

# (EXT, TABLE, SCAN): BANW with and without a table; BAXT every combination
MODES = [(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 0, 2), (1, 1, 1), (1, 1, 2)]
BUDGET = {1: 128, 2: 128, 4: 256}


@pytest.fixture(scope="module")
def units():
    names = ("dpx_bd2_kernels", "dpx_bdx_kernels", "dpx_banddir_kernels")
    isa_units.text(*names)  # they compile side by side
    return {u: {name: c[:2] for name, c in isa_units.counts(u).items()} for u in names}


def test_forty_eight_fills_a_walk_an_export_and_no_scratch(units):
    meta = units["dpx_bd2_kernels"]
    fills = {k: v for k, v in meta.items() if "k_bd2_fill" in k}
    assert len(fills) == 48, sorted(meta)
    for frag in {f"k_bd2_fillILi{c}ELb{pb}ELb{ext}ELb{tab}ELi{scan}EE" for c in (1, 2, 4) for pb in (0, 1) for ext, tab, scan in MODES}:
        assert sum(frag in k for k in fills) == 1, frag
    others = sorted(k for k in meta if k not in fills)
    assert len(others) == 2 and "k_bd2_export" in others[0] and "k_bd2_traceback" in others[1], others
    for name, (vgprs, scratch) in meta.items():
        assert scratch == 0, (name, scratch)
    for unit in ("dpx_bdx_kernels", "dpx_banddir_kernels"):  # ... and the kernels live in no other unit
        assert not any("k_bd2" in k for k in units[unit]), unit


def test_register_budget(units):
    by_mode = {}
    for name, (vgprs, _) in units["dpx_bd2_kernels"].items():
        m = re.search(r"k_bd2_fillILi(\d)ELb[01]ELb([01])ELb([01])ELi([012])EE", name)
        if m:
            by_mode.setdefault(tuple(int(x) for x in m.groups()), []).append(vgprs)
    for c in (1, 2, 4):
        counts = [v for mode in MODES for v in by_mode[(c,) + mode]]
        print(f"C={c}: k_bd2_fill {min(counts)}-{max(counts)} vgprs ({isa_units.waves_per_simd(max(counts))} waves per SIMD at the widest); "
              + ", ".join(f"(EXT={e} TABLE={t} SCAN={s}) {sorted(by_mode[c, e, t, s])}" for e, t, s in MODES))
        for mode in MODES:
            assert len(by_mode[(c,) + mode]) == 2, (c, mode)
        assert max(counts) <= BUDGET[c], (c, max(counts))
    walk = [v for k, (v, _) in units["dpx_bd2_kernels"].items() if "k_bd2_traceback" in k]
    print(f"k_bd2_traceback {walk} vgprs")
