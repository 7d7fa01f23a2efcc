"""Build-time properties of the band-direction kernels (dpx_banddir_kernels.hip) in the gfx950 code object, read from the code-object
metadata on the CPU: the unit holds exactly the 16 instantiations of k_bdir_fill, the walk and the export, none uses scratch, every
fill stays within 128 VGPRs (four waves per SIMD, the floor k_baxt_fill is held to), and no name contains a substring the other ISA
tests count their kernels by.  Metadata only: no instruction is looked at."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "csrc")
BANNED = ("k_banw", "k_baxt", "k_basw", "k_zext_fill", "k_subst", "k_asw_", "k_asg_", "k_banded_fill", "k_cigar", "k_linear_dir", "k_affine_dir")


def _metadata(isa):
    """{mangled name: (vgpr_count, private_segment_fixed_size, group_segment_fixed_size)} from the code object's kernel metadata"""
    out = {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", isa, re.S):
        block = m.group(0)
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        out[name] = tuple(int(re.search(rf"\.{key}:\s+(\d+)", block).group(1)) for key in ("vgpr_count", "private_segment_fixed_size", "group_segment_fixed_size"))
    return out


@pytest.fixture(scope="module")
def meta(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this machine")
    out = tmp_path_factory.mktemp("banddir_isa") / "dpx_banddir_kernels.s"
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(CSRC, "dpx_banddir_kernels.hip"), "-o", str(out)], check=True, timeout=900)
    return _metadata(open(out).read())


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
