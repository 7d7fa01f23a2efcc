"""ctypes access to the CPU oracle of BAXT's extension mode under a substitution table (tests/zsub_oracle.c), the five-letter table the
GPU tests use, and the fuzz set the CPU and the GPU tests share.  TEST INFRASTRUCTURE ONLY -- never imported by the product.
build(dir) compiles the oracle with `cc -O2 -shared -fPIC` into `dir` (the test modules' fixtures pass a pytest temporary directory)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import baxt_ref
import subst_ref
from zext_ref import FIELDS, NO_QUERY_END, REACHED_END, ZDROPPED, computed_mask  # noqa: F401  (re-exported for the tests)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "zsub_oracle.c")
_vp = C.c_void_p

GAPS = (-5, -1)


def acgtn_table():
    """(scores, code_of) over ACGTN: (2, -3) among ACGT, the N row and column -1 (N against N too), and one asymmetric entry: a
    reference G under a query A scores -1, a reference A under a query G keeps -3.  Lower case folds, every other byte is N."""
    scores = np.full((5, 5), -3, np.int8)
    np.fill_diagonal(scores, 2)
    scores[4, :] = -1
    scores[:, 4] = -1
    scores[2, 0] = -1  # row = reference code (G), column = query code (A)
    code = np.full(256, 4, np.uint8)
    for k, ch in enumerate(b"ACGT"):
        code[ch] = k
        code[ch + 32] = k
    return scores, code


class ZsubOracle:
    def __init__(self, path):
        lib = C.CDLL(path)
        lib.zsub_fill.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, _vp, C.c_int, _vp] + [C.c_int] * 5 + [_vp] * 9
        lib.zsub_fill.restype = C.c_int
        lib.subst_walk.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_char_p, C.c_char_p,
                                   C.c_char_p]
        lib.subst_walk.restype = C.c_int
        lib.subst_neg_inf.restype = C.c_longlong
        self.lib = lib
        self.neg_inf = lib.subst_neg_inf()

    def align(self, ref: bytes, qry: bytes, scores, code_of, gap_open: int, gap_extend: int, band: int, zdrop: int = -1,
              end_bonus: int = -1, walk: bool = True):
        """dict: rec (dpx_extension's fields by name), score and end (the chosen ones), best_cell (the scan's (bi, bj)), H, I, D (int32,
        the exported form: BAXT's with 0 where i + j > lastDiag), lines (ref, rel, qry) as bytes from the walk that starts at `end`"""
        n, m = len(ref), len(qry)
        tab = np.ascontiguousarray(scores, np.int8)
        code = np.ascontiguousarray(code_of, np.uint8)
        shape = (m + 1, n + 1)
        H, I, D = (np.zeros(shape, np.int64) for _ in range(3))
        dH, dI, dD = (np.zeros(shape, np.uint8) for _ in range(3))
        rec, chosen, bc = np.zeros(8, np.int32), np.zeros(3, np.int32), np.zeros(2, np.int32)
        rc = self.lib.zsub_fill(ref, n, qry, m, tab.ctypes.data, tab.shape[0], code.ctypes.data, gap_open, gap_extend, band, zdrop, end_bonus,
                                H.ctypes.data, I.ctypes.data, D.ctypes.data, dH.ctypes.data, dI.ctypes.data, dD.ctypes.data, rec.ctypes.data,
                                chosen.ctypes.data, bc.ctypes.data)
        assert rc == 0, rc
        r = dict(zip(FIELDS, (int(x) for x in rec)))
        keep = computed_mask(m, n, r["lastDiag"])
        eH, eI, eD = (np.where(keep, v, 0).astype(np.int32) for v in baxt_ref.exported((H, I, D), self.neg_inf, m, n, band))
        out = {"rec": r, "score": int(chosen[0]), "end": (int(chosen[1]), int(chosen[2])), "best_cell": (int(bc[0]), int(bc[1])),
               "H": eH, "I": eI, "D": eD}
        if walk:
            bufs = [C.create_string_buffer(m + n + 2) for _ in range(3)]
            k = self.lib.subst_walk(ref, n, qry, m, band, out["end"][0], out["end"][1], dH.ctypes.data, dI.ctypes.data, dD.ctypes.data, *bufs)
            assert k >= 0, "the walk left the band"
            out["lines"] = tuple(b.raw[:k] for b in bufs)
        return out

    def block(self, number: int, ref: bytes, qry: bytes, scores, code_of, gaps, band: int, zdrop: int, end_bonus: int) -> bytes:
        """the pair's text block as the output pipeline prints it ("<pair> | <score>" and three lines)"""
        r = self.align(ref, qry, scores, code_of, *gaps, band, zdrop, end_bonus)
        return b"%d | %d\n" % (number, r["score"]) + b"".join(x + b"\n" for x in r["lines"])


def build(out_dir) -> ZsubOracle:
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    so = os.path.join(str(out_dir), "libzsub_oracle.so")
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-o", so, SRC], check=True)
    return ZsubOracle(so)


# the fuzz set shared by the CPU and the GPU tests: two letters, m and n in 0..13, bands 1..5 (40 pairs each), subst_ref's four tables
# and gap weights, Z in {0, 2, 6} with E = 3.  The seed is chosen so that the set holds every class tests/test_zsub_oracle.py asserts.
FUZZ_TABLES, FUZZ_GAPS = subst_ref.FUZZ_TABLES, subst_ref.FUZZ_GAPS
FUZZ_Z, FUZZ_E, FUZZ_BANDS, FUZZ_SEED = (0, 2, 6), 3, range(1, 6), 126


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
