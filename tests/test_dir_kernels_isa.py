"""Build-time properties of the direction-matrix kernels (dpx_dir_kernels.hip), checked on the CPU: no scratch memory, no matrix cores,
fill kernels within 128 VGPRs, and every store of a fill kernel a whole dword or wider (the codes leave as one 16-byte store per lane and
group of steps: whole 64-byte sectors)."""
import re

import pytest

import isa_units

WIDE = {"global_store_dword", "global_store_dwordx2", "global_store_dwordx3", "global_store_dwordx4"}


@pytest.fixture(scope="module")
def isa():
    return isa_units.text("dpx_dir_kernels")


def _kernels(isa):
    """{mangled name: (metadata text, body text)}"""
    return {name: v[:2] for name, v in isa_units.kernels("dpx_dir_kernels").items()}


def _fills(ks):
    return {k: v for k, v in ks.items() if "k_linear_dir" in k or "k_affine_dir" in k}


def test_no_scratch_no_mfma(isa):
    ks = _kernels(isa)
    assert len(_fills(ks)) == 20, sorted(ks)  # (LNW at 2/4/8/16 rows per lane, LSW and ANW at 2/4/8) x (edge rows in LDS / in global memory)
    for name, (meta, body) in ks.items():
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", meta), name
        assert "scratch_" not in body, name
    assert "v_mfma" not in isa


def test_fill_kernels_fit_128_vgprs(isa):
    for name, (meta, _) in _fills(_kernels(isa)).items():
        assert isa_units.vgprs(meta) <= 128, name


def test_fill_stores_are_dword_or_wider(isa):
    for name, (_, body) in _fills(_kernels(isa)).items():
        stores = isa_units.stores(body)
        assert stores, name
        assert stores <= WIDE, (name, stores - WIDE)
        assert "global_store_dwordx4" in stores, name  # the codes: one 16-byte store per lane and group of steps
        assert "v_mov_b32_dpp" in body, name           # `up` of the top row from the lane above
