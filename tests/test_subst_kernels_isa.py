"""Build-time properties of the substitution-table kernels (dpx_subst_kernels.hip) in the gfx950 code object, read from the code-object
metadata on the CPU: the unit holds exactly the 32 instantiations of k_subst_fill and the two walks, none uses scratch, every fill
stays within 128 VGPRs (four waves per SIMD, the floor k_baxt_fill is held to), and no name contains a substring the other ISA tests
count their kernels by."""
import re

import pytest

import isa_units

BANNED = ("k_banw", "k_baxt", "k_basw", "k_zext_fill", "k_asw_", "k_asg_", "k_banded_fill", "k_cigar")


@pytest.fixture(scope="module")
def meta():
    """{mangled name: (vgpr_count, private_segment_fixed_size)} from the code object's kernel metadata"""
    return {name: c[:2] for name, c in isa_units.counts("dpx_subst_kernels").items()}


def test_thirty_two_fills_two_walks_and_no_scratch(meta):
    fills = {k: v for k, v in meta.items() if "k_subst_fill" in k}
    walks = sorted(k for k in meta if "k_subst_fill" not in k)
    assert len(meta) == 34 and len(fills) == 32, sorted(meta)
    assert len(walks) == 2 and "17k_subst_tracebackE" in walks[0] and "22k_subst_traceback_waveE" in walks[1], walks
    for frag in {f"k_subst_fillILi{c}ELb{pb}ELb{st}ELb{ext}EE" for c in (1, 2, 4, 8) for pb in (0, 1) for st in (0, 1) for ext in (0, 1)}:
        assert sum(frag in k for k in meta) == 1, frag
    for name, (vgprs, scratch) in meta.items():
        assert scratch == 0, (name, scratch)
        for banned in BANNED:
            assert banned not in name, name


def test_fills_keep_four_waves_per_simd(meta):
    by_c = {}
    for name, (vgprs, _) in meta.items():
        m = re.search(r"k_subst_fillILi(\d)ELb[01]ELb[01]ELb([01])EE", name)
        if m:
            by_c.setdefault((int(m.group(1)), int(m.group(2))), []).append(vgprs)
    for c in (1, 2, 4, 8):
        print(f"C={c}: k_subst_fill BANW end {sorted(by_c[c, 0])}, BAXT end {sorted(by_c[c, 1])} vgprs")
        assert len(by_c[c, 0]) == len(by_c[c, 1]) == 4
        assert max(by_c[c, 0] + by_c[c, 1]) <= 128, (c, by_c[c, 0], by_c[c, 1])
