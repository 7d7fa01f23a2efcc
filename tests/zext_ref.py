"""ctypes access to the CPU oracle of BAXT's extension mode (tests/zext_oracle.c).  TEST INFRASTRUCTURE ONLY -- never imported by
the product.  build(dir) compiles it with `cc -O2 -shared -fPIC` into `dir` (the test modules' fixtures pass a pytest temporary
directory)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import baxt_ref

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "zext_oracle.c")
_vp = C.c_void_p
ZDROPPED, REACHED_END = 1, 2
NO_QUERY_END = -2**31
FIELDS = ("maxScore", "maxRow", "maxCol", "qryEndScore", "qryEndCol", "lastDiag", "flags", "reserved")


def computed_mask(m: int, n: int, last_diag: int) -> np.ndarray:
    """(m+1) x (n+1) bool: i + j <= lastDiag"""
    i, j = np.mgrid[0:m + 1, 0:n + 1]
    return i + j <= last_diag


class ZextOracle:
    def __init__(self, path):
        lib = C.CDLL(path)
        lib.zext_fill.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int] + [C.c_int] * 7 + [_vp] * 9
        lib.zext_fill.restype = C.c_int
        lib.baxt_walk.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_char_p, C.c_char_p,
                                  C.c_char_p, _vp, _vp]
        lib.baxt_walk.restype = C.c_int
        lib.baxt_neg_inf.restype = C.c_longlong
        self.lib = lib
        self.neg_inf = lib.baxt_neg_inf()

    def align(self, ref: bytes, qry: bytes, match: int, mismatch: int, gap_open: int, gap_extend: int, band: int, zdrop: int = -1,
              end_bonus: int = -1, walk: bool = True):
        """dict: rec (dpx_extension's fields by name), score and end (the chosen ones), best_cell (the scan's (bi, bj)), H, I, D (int32,
        the exported form: BAXT's with 0 where i + j > lastDiag), lines (ref, rel, qry) as bytes from BANW's walk"""
        n, m = len(ref), len(qry)
        shape = (m + 1, n + 1)
        H, I, D = (np.zeros(shape, np.int64) for _ in range(3))
        dH, dI, dD = (np.zeros(shape, np.uint8) for _ in range(3))
        rec, chosen, bc = np.zeros(8, np.int32), np.zeros(3, np.int32), np.zeros(2, np.int32)
        rc = self.lib.zext_fill(ref, n, qry, m, match, mismatch, gap_open, gap_extend, band, zdrop, end_bonus, H.ctypes.data, I.ctypes.data,
                                D.ctypes.data, dH.ctypes.data, dI.ctypes.data, dD.ctypes.data, rec.ctypes.data, chosen.ctypes.data,
                                bc.ctypes.data)
        assert rc == 0, rc
        r = dict(zip(FIELDS, (int(x) for x in rec)))
        keep = computed_mask(m, n, r["lastDiag"])
        eH, eI, eD = (np.where(keep, v, 0).astype(np.int32) for v in baxt_ref.exported((H, I, D), self.neg_inf, m, n, band))
        out = {"rec": r, "score": int(chosen[0]), "end": (int(chosen[1]), int(chosen[2])), "best_cell": (int(bc[0]), int(bc[1])),
               "H": eH, "I": eI, "D": eD}
        if walk:
            bufs = [C.create_string_buffer(m + n + 2) for _ in range(3)]
            cells = np.zeros((m + n + 1, 2), np.int32)
            nc = C.c_int32()
            k = self.lib.baxt_walk(ref, n, qry, m, band, out["end"][0], out["end"][1], dH.ctypes.data, dI.ctypes.data, dD.ctypes.data, *bufs,
                                   cells.ctypes.data, C.addressof(nc))
            assert k >= 0, "the walk left the band"
            assert all(i + j <= r["lastDiag"] for i, j in cells[:nc.value]), "the walk left the computed cells"
            out["lines"] = tuple(b.raw[:k] for b in bufs)
        return out

    def block(self, number: int, ref: bytes, qry: bytes, w, band: int, zdrop: int, end_bonus: int) -> bytes:
        """the pair's text block as the output pipeline prints it ("<pair> | <score>" and three lines)"""
        r = self.align(ref, qry, *w, band, zdrop, end_bonus)
        return b"%d | %d\n" % (number, r["score"]) + b"".join(x + b"\n" for x in r["lines"])


def build(out_dir) -> ZextOracle:
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    so = os.path.join(str(out_dir), "libzext_oracle.so")
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-o", so, SRC], check=True)
    return ZextOracle(so)


# the fuzz set shared by the CPU and the GPU tests: two letters, m and n in 0..13, bands 1..5 (40 pairs each), BAXT's six weight sets,
# Z in {0, 2, 6} with E = 3.  The seed is chosen so that, under the weights (2, -1, 1, -1), at least one pair's scan cell (bi, bj)
# differs from (maxRow, maxCol) (tests/test_zext_oracle.py asserts it).
FUZZ_WEIGHTS = [(3, -1, -3, -1), (1, -1, -1, -1), (2, -3, -5, -1), (1, -2, 0, -1), (2, -1, 1, -1), (1, -1, -3, 2)]
FUZZ_Z, FUZZ_E, FUZZ_BANDS, FUZZ_SEED = (0, 2, 6), 3, range(1, 6), 77


def fuzz_texts(seed: int = FUZZ_SEED):
    """{band: [(ref, qry)] * 40}"""
    rng = np.random.default_rng(seed)
    out = {}
    for band in FUZZ_BANDS:
        texts = []
        for _ in range(40):
            n, m = int(rng.integers(0, 14)), int(rng.integers(0, 14))
            texts.append((rng.integers(65, 67, n).astype(np.uint8).tobytes(), rng.integers(65, 67, m).astype(np.uint8).tobytes()))
        out[band] = texts
    return out
