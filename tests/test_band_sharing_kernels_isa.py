"""The five BANW-family translation units (dpx_banw / dpx_baxt / dpx_zext / dpx_subst / dpx_banddir _kernels.hip) after they came to share
dpx_band_affine.hpp, against tests/golden/kernel_vgprs_before_band_sharing.json (mangled name -> .vgpr_count, from the commit before):
every unit still holds exactly the kernels it held, none uses scratch, and no kernel runs fewer waves per SIMD than it did.  Metadata
only: no instruction is looked at."""
import json
import os

import isa_units


_waves_per_simd = isa_units.waves_per_simd


def test_same_kernels_no_scratch_and_no_fewer_waves_per_simd():
    golden = json.load(open(os.path.join(isa_units.ROOT, "tests", "golden", "kernel_vgprs_before_band_sharing.json")))["kernels"]
    assert sorted(golden) == ["dpx_banddir_kernels.hip", "dpx_banw_kernels.hip", "dpx_baxt_kernels.hip", "dpx_subst_kernels.hip", "dpx_zext_kernels.hip"]
    isa_units.text(*golden)  # the five compile side by side
    for unit, want in golden.items():
        got = {name: c[:2] for name, c in isa_units.counts(unit).items()}
        assert sorted(got) == sorted(want), (unit, sorted(set(got) ^ set(want)))
        for name, (vgprs, scratch) in got.items():
            print(f"{unit} {name}: {want[name]} -> {vgprs} vgprs")
            assert scratch == 0, (unit, name, scratch)
            assert _waves_per_simd(vgprs) >= _waves_per_simd(want[name]), (unit, name, want[name], vgprs)
