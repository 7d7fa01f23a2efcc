"""The buffer caches and the owning buffer handle (csrc/dpx_mem.h) on the CPU: tests/bufcache_main.cpp, a stand-alone program, is compiled
with the host compiler together with csrc/dpx_mem.cpp and csrc/dpx_host.cpp under the address and undefined-behaviour sanitizers, linked
against the HIP runtime alone (no kernel unit), and run.  Its caches stand on a fake allocator of never-dereferenced addresses, so the
take window, the three roofs, the per-device rule, the park limits, the GiB rules, the retry after out-of-memory, drain and every
operation of the handle are pinned without a device; a double free, a free of an unknown address or a sanitizer report fails it."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ROCM = os.path.dirname(os.path.dirname(os.path.realpath(HIPCC)))


def test_bufcache_and_handle_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = tmp_path / "bufcache"
    sources = [os.path.join(ROOT, "tests", "bufcache_main.cpp"), os.path.join(CSRC, "dpx_mem.cpp"), os.path.join(CSRC, "dpx_host.cpp")]
    libdir = os.path.join(ROCM, "lib")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, "-I", os.path.join(ROCM, "include"), *sources, "-o", str(exe),
                    "-L", libdir, "-Wl,-rpath," + libdir, "-lamdhip64", "-lpthread"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and r.stdout.endswith(" checks\n"), (r.stdout, r.stderr)
    assert r.stderr == "", r.stderr  # no sanitizer report
