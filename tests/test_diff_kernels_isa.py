"""Build-time properties of the difference-string kernels (dpx_diff_kernels.hip) in the gfx950 code object, read from the code-object
metadata on the CPU: the unit compiles, every kernel in it is a k_diff_* kernel whose name holds none of the substrings the other ISA
tests count kernels by, and none of them uses scratch."""
import re

import pytest

import isa_units
from test_cigar_kernels_isa import COUNTED_ELSEWHERE


@pytest.fixture(scope="module")
def meta():
    """{mangled name: private_segment_fixed_size} from the code object's kernel metadata"""
    return {name: c[1] for name, c in isa_units.counts("dpx_diff_kernels").items()}


def test_the_unit_holds_the_three_stages(meta):
    for stage in ("k_diff_count", "k_diff_scan", "k_diff_write"):
        assert any(stage in name for name in meta), (stage, sorted(meta))
    assert sum("k_diff_count" in name for name in meta) == 2 and sum("k_diff_write" in name for name in meta) == 2  # one per kind


def test_every_kernel_is_a_diff_kernel(meta):
    for name in meta:
        assert re.search(r"\d+k_diff_[a-z_]+", name), name  # (Itanium mangling: <length><identifier>)
        assert "k_cigar" not in name, name
        for banned in COUNTED_ELSEWHERE:
            assert banned not in name, (name, banned)


def test_no_kernel_uses_scratch(meta):
    for name, scratch in meta.items():
        assert scratch == 0, (name, scratch)
