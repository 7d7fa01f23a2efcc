"""The direction-code layout (csrc/dpx_dir.h) on the CPU: a small host program walks the index function over whole matrices -- every rows
per lane value, query lengths around one and two stripes, reference lengths 1..40 (every residue of the store group), a pair alone and
interleaved with two others -- and checks that the cells with i, j >= 1 get distinct nibbles inside the pair's chunks x 1024 bytes, that
the header's formula holds term by term, and that the chunk count is stripes x (steps of a stripe / steps of a store group)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
ROCM_INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(HIPCC))), "include")
ROWS = (2, 4, 8, 16)

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dpx_dir.h"
int main(int argc, char **argv) {
    const int R = atoi(argv[1]);
    const int G = dpx_dir_group(R);
    if (G != 32 / R || G * R != 32) { printf("group %d\n", G); return 1; }
    const int ms[] = {1, 64 * R - 1, 64 * R, 64 * R + 1, 128 * R + 1};
    long cellsSeen = 0;
    for (const int m : ms)
        for (int n = 1; n <= 40; n++) {
            const unsigned long long stripes = (unsigned long long)(m + 64 * R - 1) / (64 * R);
            const unsigned long long Wp = dpx_dir_stripe_steps(n, R);
            if (Wp % G || Wp < (unsigned long long)n + 63 || Wp >= (unsigned long long)n + 63 + G) { printf("steps %d %d: %llu\n", R, n, Wp); return 1; }
            const unsigned long long chunks = dpx_dir_chunks(m, n, R);
            if (chunks != stripes * (Wp / G)) { printf("chunks %d %d %d: %llu\n", R, m, n, chunks); return 1; }
            for (const unsigned long long stride : {1024ull, 3 * 1024ull}) { /* alone, and interleaved with two other pairs */
                std::vector<unsigned char> seen(chunks * 1024 * 2, 0); /* one flag per nibble */
                for (int i = 1; i <= m; i++)
                    for (int j = 1; j <= n; j++) {
                        int shift = -1;
                        const unsigned long long off = dpx_dir_byte(i, j, n, R, stride, &shift);
                        if (shift != 0 && shift != 4) { printf("shift %d\n", shift); return 1; }
                        const unsigned long long chunk = off / stride, inside = off % stride;
                        if (chunk >= chunks || inside >= 1024) { printf("outside %d %d %d (%d, %d): %llu\n", R, m, n, i, j, off); return 1; }
                        const unsigned long long at = (chunk * 1024 + inside) * 2 + (shift >> 2);
                        if (seen[at]) { printf("twice %d %d %d (%d, %d)\n", R, m, n, i, j); return 1; }
                        seen[at] = 1;
                        /* the formula of the header, term by term */
                        const int i0 = i - 1, k = i0 / (64 * R), l = (i0 / R) % 64, r = i0 % R;
                        const unsigned long long T = (unsigned long long)k * Wp + (unsigned long long)(j - 1) + l;
                        const int nib = (int)(T % G) * R + r;
                        if (off != (T / G) * stride + l * 16 + nib / 2 || shift != (nib & 1) * 4) { printf("formula %d %d %d (%d, %d)\n", R, m, n, i, j); return 1; }
                        if (T / G < (unsigned long long)k * (Wp / G) || T / G >= (unsigned long long)(k + 1) * (Wp / G)) { printf("stripe %d %d %d (%d, %d)\n", R, m, n, i, j); return 1; }
                        cellsSeen++;
                    }
            }
        }
    if (dpx_dir_chunks(0, 5, R) || dpx_dir_chunks(5, 0, R) || dpx_dir_chunks(0, 0, R)) { printf("empty\n"); return 1; }
    printf("ok %d G=%d cells=%ld\n", R, G, cellsSeen);
    return 0;
}
"""


def test_header_constants():
    header = open(os.path.join(CSRC, "dpx_dir.h")).read()
    assert "#define DPX_DIR_CHUNK_BYTES 1024u" in header and "#define DPX_DIR_SCRATCH_SLOTS 2048" in header


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    d = tmp_path_factory.mktemp("dir_layout")
    src, exe = d / "layout.cpp", d / "layout"
    src.write_text(PROGRAM)
    # (the header pulls in hip/hip_runtime.h through dpx_kernels.h: host compiler, AMD platform, ROCm's include directory)
    subprocess.run([cxx, "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", CSRC, "-I", ROCM_INCLUDE, str(src), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("rows", ROWS)
def test_index_function(program, rows):
    r = subprocess.run([program, str(rows)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith(f"ok {rows} G={32 // rows} "), (r.stdout, r.stderr)
    cells = 2 * sum(m * n for m in (1, 64 * rows - 1, 64 * rows, 64 * rows + 1, 128 * rows + 1) for n in range(1, 41))
    assert f"cells={cells}\n" in r.stdout, r.stdout
