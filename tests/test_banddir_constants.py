"""The band-direction layout (csrc/dpx_banddir.h) and the Python constant, on the CPU: a small host program walks the index function
over whole bands and checks that the in-band cells with i, j >= 1 get distinct nibbles, that every one of them lies inside the pair's
chunks x 1024 bytes, and that the chunk count is ceil((m + n - 1) / (32 / C))."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "csrc")
BANDS = (1, 2, 17, 64, 65, 129, 257, 512)

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "dpx_banddir.h"
int main(int argc, char **argv) {
    const int B = atoi(argv[1]);
    const int C = dpx_band_cpl(B), Gd = dpx_banddir_group(C);
    const int shapes[][2] = {{1, 1}, {1, B}, {B, 1}, {B + 3, B + 3}, {2 * B + 40, 2 * B + 11}, {2 * B + 7, 2 * B + 40}, {B + 40, 5}, {31, 2 * B + 40}};
    long cellsSeen = 0;
    for (const auto &sh : shapes) {
        const int m = sh[0], n = sh[1];
        const unsigned long long chunks = dpx_banddir_chunks(m, n, B);
        if (chunks != ((unsigned long long)(m + n - 1) + Gd - 1) / Gd) { printf("chunks %d %d %d: %llu\n", B, m, n, chunks); return 1; }
        for (const unsigned long long stride : {1024ull, 3 * 1024ull}) { /* alone, and interleaved with two other pairs */
            std::vector<unsigned char> seen(chunks * 1024 * 2, 0); /* one flag per nibble */
            for (int i = 1; i <= m; i++)
                for (int j = 1; j <= n; j++) {
                    if (abs(i - j) > B - 1) continue;
                    int shift = -1;
                    const unsigned long long off = dpx_banddir_byte(i, j, B, stride, &shift);
                    if (shift != 0 && shift != 4) { printf("shift %d\n", shift); return 1; }
                    const unsigned long long chunk = off / stride, inside = off % stride;
                    if (chunk >= chunks || inside >= 1024) { printf("outside %d %d %d (%d, %d): %llu\n", B, m, n, i, j, off); return 1; }
                    const unsigned long long nib = (chunk * 1024 + inside) * 2 + (shift >> 2);
                    if (seen[nib]) { printf("twice %d %d %d (%d, %d)\n", B, m, n, i, j); return 1; }
                    seen[nib] = 1;
                    /* the formula of the header, term by term */
                    const int A = i + j - 2, s = (i - j + B - 1) >> 1, l = s / C, c = s % C, nb = (A % Gd) * C + c;
                    if (off != (unsigned long long)(A / Gd) * stride + l * 16 + nb / 2 || shift != (nb & 1) * 4) { printf("formula\n"); return 1; }
                    if (off < dpx_banddir_piece(A / Gd, l, stride) || off >= dpx_banddir_piece(A / Gd, l, stride) + 16) { printf("piece\n"); return 1; }
                    cellsSeen++;
                }
        }
    }
    if (dpx_banddir_chunks(0, 5, B) || dpx_banddir_chunks(5, 0, B)) return 1;
    printf("ok %d C=%d Gd=%d cells=%ld\n", B, C, Gd, cellsSeen);
    return 0;
}
"""


def test_public_constant_and_header():
    import dpx_gpu_genomics_project_amd as dpx

    assert dpx.KEEP_BAND_DIRECTIONS == 0x10 and dpx.capi.KEEP_BAND_DIRECTIONS == 0x10 and "KEEP_BAND_DIRECTIONS" in dpx.__all__
    assert dpx.KEEP_DIRECTIONS == 0x8
    header = open(os.path.join(ROOT, "include", "dpx_align.h")).read()
    assert re.search(r"#define\s+DPX_KEEP_BAND_DIRECTIONS\s+0x10u\b", header)
    assert "#define DPX_ABI_VERSION 3" in header
    assert "k_banw_fill / k_baxt_fill" in header and "DPX_ERR_NO_MATRIX" in header  # how a caller detects the flag


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    d = tmp_path_factory.mktemp("banddir_layout")
    src, exe = d / "layout.cpp", d / "layout"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-O1", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("band", BANDS)
def test_index_function(program, band):
    r = subprocess.run([program, str(band)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith(f"ok {band} "), (r.stdout, r.stderr)
    c = 1 if band <= 64 else 2 if band <= 128 else 4 if band <= 256 else 8
    assert f"C={c} Gd={32 // c} " in r.stdout, r.stdout
