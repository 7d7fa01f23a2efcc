"""Build-time properties of the CIGAR kernels (dpx_cigar_kernels.hip) in the gfx950 code object, read from the code-object metadata on
the CPU: the unit compiles, every kernel in it is a k_cigar_* kernel whose name holds none of the substrings the other ISA tests
count kernels by, and none of them uses scratch."""
import re

import pytest

import isa_units

COUNTED_ELSEWHERE = ("k_basw", "k_banw", "k_baxt", "k_asw_", "k_asg_", "k_banded_fill", "k_linear_dir", "k_affine_dir", "k_traceback_wave")


@pytest.fixture(scope="module")
def meta():
    """{mangled name: private_segment_fixed_size} from the code object's kernel metadata"""
    return {name: c[1] for name, c in isa_units.counts("dpx_cigar_kernels").items()}


def test_the_unit_holds_the_three_stages(meta):
    for stage in ("k_cigar_count", "k_cigar_scan", "k_cigar_write"):
        assert any(stage in name for name in meta), (stage, sorted(meta))


def test_every_kernel_is_a_cigar_kernel(meta):
    for name in meta:
        assert re.search(r"\d+k_cigar_[a-z_]+", name), name  # (Itanium mangling: <length><identifier>)
        for banned in COUNTED_ELSEWHERE:
            assert banned not in name, (name, banned)


def test_no_kernel_uses_scratch(meta):
    for name, scratch in meta.items():
        assert scratch == 0, (name, scratch)
