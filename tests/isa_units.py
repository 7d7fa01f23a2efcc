"""The gfx950 listings of csrc/'s kernel units for the test_*isa*.py files: every unit is compiled at most once per pytest process
(hipcc cross-compiles without a GPU), several at a time when several are asked for, and parsed once.

A unit is named with or without ".hip".  "dpx_kernels.hip" once held the kernels of five families; whoever asks for it (a test, or a
golden file keyed by it) gets the units that succeeded it, SUCCESSORS."""
import functools
import os
import re
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "csrc")
SUCCESSORS = {"dpx_kernels.hip": ("dpx_kernels.hip", "dpx_affine_kernels.hip", "dpx_bsw_kernels.hip", "dpx_traceback_kernels.hip",
                                  "dpx_output_kernels.hip")}
STORES = r"\b(global_store_\w+|buffer_store_\w+|flat_store_\w+)"


def _files(units):
    """the unit files behind the names asked for, each once, in order"""
    out = []
    for unit in units:
        unit = unit if unit.endswith(".hip") else unit + ".hip"
        out += [u for u in SUCCESSORS.get(unit, (unit,)) if u not in out]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _listing(unit):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc on this machine")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, unit[:-4] + ".s")
        subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                        os.path.join(CSRC, unit), "-o", out], check=True, timeout=900)
        return open(out).read()


@functools.lru_cache(maxsize=None)
def _parsed(unit):
    """{mangled name: (metadata, body, unit)}: the kernel's block of the code-object metadata and its text from label to .Lfunc_end"""
    isa, out = _listing(unit), {}
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", isa, re.S):
        name = re.search(r"\.name:\s+(\S+)", m.group(0)).group(1)
        start = isa.find("\n" + name + ":")
        out[name] = (m.group(0), isa[start:isa.find(".Lfunc_end", start)] if start >= 0 else "", unit)
    return out


def text(*units):
    """the listings of the units, concatenated; at most 8 compile side by side"""
    files = _files(units)
    with ThreadPoolExecutor(max_workers=8) as pool:
        return "\n".join(pool.map(_listing, files))


def kernels(*units):
    """{mangled name: (metadata, body, unit)} over the units; no kernel may be in two of them"""
    text(*units)
    out = {}
    for unit in _files(units):
        for name, entry in _parsed(unit).items():
            assert name not in out, (name, out[name][2], unit)
            out[name] = entry
    return out


def counts(*units):
    """{mangled name: (vgpr_count, private_segment_fixed_size, group_segment_fixed_size)}, for the tests that read metadata only"""
    return {name: tuple(field(meta, key) for key in ("vgpr_count", "private_segment_fixed_size", "group_segment_fixed_size"))
            for name, (meta, _, _) in kernels(*units).items()}


def waves_per_simd(vgprs):
    """gfx950: 512 registers per lane and SIMD, allocated in blocks of 8, at most 8 waves"""
    return min(8, 512 // ((vgprs + 7) // 8 * 8))


def field(meta, key):
    return int(re.search(rf"\.{key}:\s+(\d+)", meta).group(1))


def vgprs(meta):
    return field(meta, "vgpr_count")


def stores(body):
    return set(re.findall(STORES, body))
