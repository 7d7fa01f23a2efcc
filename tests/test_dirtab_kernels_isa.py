"""Build-time properties of k_dirtab_fill (dpx_dirtab_kernels.hip: ANW / ASW / ASG direction batches under
dpx_batch_set_direction_table) in the gfx950 code object, read from the code-object metadata on the CPU: the unit holds exactly the 18
instantiations (3 kinds x 3 rows per lane x edge rows in LDS / in global memory) and nothing else, none uses scratch, every fill stays
within 128 VGPRs at R = 2 and 4 and within 168 (three waves per SIMD, the floor k_bdx_fill is held to at C = 8) at R = 8, and no
k_dirtab kernel lives in dpx_dir_kernels.  The counts are printed beside the plain kernels' at the same R.  Metadata only: no
instruction is looked at."""
import re

import pytest

import isa_units

KINDS = {2: ("ANW", "k_affine_dir"), 4: ("ASW", "k_asw_dir"), 6: ("ASG", "k_asg_dir")}  # DPX_K_ANW / _ASW / _ASG: the KIND argument


@pytest.fixture(scope="module")
def units():
    names = ("dpx_dirtab_kernels", "dpx_dir_kernels")
    isa_units.text(*names)  # the two compile side by side
    return {u: {name: c[:2] for name, c in isa_units.counts(u).items()} for u in names}


def test_eighteen_fills_nothing_else_and_no_scratch(units):
    meta = units["dpx_dirtab_kernels"]
    assert len(meta) == 18 and all("k_dirtab_fill" in k for k in meta), sorted(meta)
    for frag in {f"k_dirtab_fillILi{r}ELb{g}ELi{kind}EE" for r in (2, 4, 8) for g in (0, 1) for kind in KINDS}:
        assert sum(frag in k for k in meta) == 1, frag
    for name, (vgprs, scratch) in meta.items():
        assert scratch == 0, (name, scratch)
        for banned in ("k_linear_dir", "k_affine_dir", "k_asw_", "k_asg_", "k_bdx", "k_bdir", "k_subst", "k_zsub"):  # substrings the other ISA tests count kernels by
            assert banned not in name, name
    assert not any("k_dirtab" in k for k in units["dpx_dir_kernels"])  # ... and the kernel lives in no other unit


def test_register_budget(units):
    tab, plain = {}, {}
    for name, (vgprs, _) in units["dpx_dirtab_kernels"].items():
        r, kind = re.search(r"k_dirtab_fillILi(\d)ELb[01]ELi(\d)EE", name).groups()
        tab.setdefault((int(r), int(kind)), []).append(vgprs)
    for name, (vgprs, _) in units["dpx_dir_kernels"].items():
        for kind, (_, kernel) in KINDS.items():
            m = re.search(kernel + r"ILi(\d)ELb[01]EE", name)
            if m:
                plain.setdefault((int(m.group(1)), kind), []).append(vgprs)
    for r in (2, 4, 8):
        print(f"R={r}: " + ", ".join(f"{KINDS[k][0]} {KINDS[k][1]} {sorted(plain[r, k])} k_dirtab_fill {sorted(tab[r, k])} vgprs" for k in KINDS))
        for kind in KINDS:
            assert len(tab[r, kind]) == 2 and len(plain[r, kind]) == 2, (r, kind)
            assert max(tab[r, kind]) <= (168 if r == 8 else 128), (r, kind, tab[r, kind])
