"""Build-time properties of the orientation kernels (dpx_reverse_kernels.hip: k_reverse_strings, k_flip_lines, k_map_records) in the
gfx950 code object, read from the code-object metadata on the CPU: the unit holds exactly these three kernels, none of them uses scratch
or LDS, and each keeps eight waves per SIMD.  The register counts are printed.  Metadata only: no instruction is looked at."""
import pytest

import isa_units

KERNELS = ("k_reverse_strings", "k_flip_lines", "k_map_records")


@pytest.fixture(scope="module")
def meta():
    return isa_units.counts("dpx_reverse_kernels")


def test_three_kernels_without_scratch_or_lds(meta):
    assert len(meta) == 3, sorted(meta)
    for kernel in KERNELS:
        assert sum(kernel in name for name in meta) == 1, (kernel, sorted(meta))
    for name, (vgprs, scratch, lds) in meta.items():
        assert scratch == 0 and lds == 0, (name, scratch, lds)


def test_register_counts(meta):
    for kernel in KERNELS:
        vgprs = next(v for name, (v, _, _) in meta.items() if kernel in name)
        print(f"{kernel}: {vgprs} vgprs, {isa_units.waves_per_simd(vgprs)} waves per SIMD")
        assert isa_units.waves_per_simd(vgprs) == 8, (kernel, vgprs)   # (at most 64 registers: memory-bound passes, latency hidden by occupancy)
