"""Build-time properties of the band-direction kernels (dpx_banddir_kernels.hip) in the gfx950 code object, read from the code-object
metadata on the CPU: the unit holds exactly the 16 instantiations of k_bdir_fill, the walk and the export, none uses scratch, every
fill stays within 128 VGPRs (four waves per SIMD, the floor k_baxt_fill is held to), and no name contains a substring the other ISA
tests count their kernels by.  Metadata only: no instruction is looked at."""
import re

import pytest

import isa_units

BANNED = ("k_banw", "k_baxt", "k_basw", "k_zext_fill", "k_subst", "k_asw_", "k_asg_", "k_banded_fill", "k_cigar", "k_linear_dir", "k_affine_dir")


@pytest.fixture(scope="module")
def meta():
    """{mangled name: (vgpr_count, private_segment_fixed_size, group_segment_fixed_size)} from the code object's kernel metadata"""
    return isa_units.counts("dpx_banddir_kernels")


def test_sixteen_fills_one_walk_one_export_and_no_scratch(meta):
    fills = {k: v for k, v in meta.items() if "k_bdir_fill" in k}
    others = sorted(k for k in meta if "k_bdir_fill" not in k)
    assert len(meta) == 18 and len(fills) == 16, sorted(meta)
    assert len(others) == 2 and "13k_bdir_exportE" in others[0] and "16k_bdir_tracebackE" in others[1], others
    for frag in {f"k_bdir_fillILi{c}ELb{pb}ELb{ext}EE" for c in (1, 2, 4, 8) for pb in (0, 1) for ext in (0, 1)}:
        assert sum(frag in k for k in meta) == 1, frag
    for name, (vgprs, scratch, lds) in meta.items():
        assert scratch == 0, (name, scratch)
        for banned in BANNED:
            assert banned not in name, name
    walk = next(v for k, v in meta.items() if "k_bdir_traceback" in k)
    assert walk[2] == 16 * 1024, walk  # the ring of sixteen 1-KiB chunks


def test_fills_keep_four_waves_per_simd(meta):
    by_c = {}
    for name, (vgprs, _, _) in meta.items():
        m = re.search(r"k_bdir_fillILi(\d)ELb[01]ELb([01])EE", name)
        if m:
            by_c.setdefault((int(m.group(1)), int(m.group(2))), []).append(vgprs)
    for c in (1, 2, 4, 8):
        print(f"C={c}: k_bdir_fill BANW end {sorted(by_c[c, 0])}, BAXT end {sorted(by_c[c, 1])} vgprs")
        assert len(by_c[c, 0]) == len(by_c[c, 1]) == 2
        assert max(by_c[c, 0] + by_c[c, 1]) <= 128, (c, by_c[c, 0], by_c[c, 1])
    for name, (vgprs, _, _) in meta.items():
        if "k_bdir_fill" not in name:
            print(f"{name}: {vgprs} vgprs")
