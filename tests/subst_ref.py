"""ctypes access to the substitution-table CPU oracle (tests/subst_oracle.c), plus an independent NumPy fill and the host's range
bounds.  TEST INFRASTRUCTURE ONLY -- never imported by the product.  build(dir) compiles the oracle with `cc -O2 -shared -fPIC` into
`dir` (the test modules' fixtures pass a pytest temporary directory)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from baxt_ref import band_mask, exported

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "subst_oracle.c")
_vp = C.c_void_p


def identity_table(match: int, mismatch: int, used: bytes):
    """(scores, code_of) that score exactly as byte equality does over the distinct bytes of `used` (at most 32): an injective map"""
    letters = sorted(set(used)) or [65]
    assert len(letters) <= 32
    code = np.zeros(256, np.uint8)
    for k, ch in enumerate(letters):
        code[ch] = k
    a = len(letters)
    scores = np.full((a, a), mismatch, np.int8)
    np.fill_diagonal(scores, match)
    return scores, code


def numpy_fill(ref: bytes, qry: bytes, scores, code_of, gap_open: int, gap_extend: int, band: int):
    """H, I, D as int64 (m+1) x (n+1) with NEG for minus infinity, filled anti-diagonal by anti-diagonal with array operations (the
    oracle goes row by row): an independent second implementation of the definition"""
    NEG = -(1 << 40)
    n, m = len(ref), len(qry)
    code = np.asarray(code_of, np.int64)
    rc, qc = code[np.frombuffer(ref, np.uint8)], code[np.frombuffer(qry, np.uint8)]
    s = np.asarray(scores, np.int64)[rc[None, :], qc[:, None]]  # (m, n): row of the table = reference code
    H, I, D = (np.full((m + 1, n + 1), NEG, np.int64) for _ in range(3))
    inb = band_mask(m, n, band)
    H[0, 0] = 0
    for i in range(1, m + 1):
        if inb[i, 0]:
            H[i, 0] = gap_open + i * gap_extend
    for j in range(1, n + 1):
        if inb[0, j]:
            H[0, j] = gap_open + j * gap_extend
    plus = lambda a, w: np.where(a == NEG, NEG, a + w)
    for a in range(2, m + n + 1):
        i = np.arange(max(1, a - n), min(m, a - 1) + 1)
        j = a - i
        keep = inb[i, j]
        i, j = i[keep], j[keep]
        if not i.size:
            continue
        D[i, j] = np.maximum(plus(H[i - 1, j], gap_open + gap_extend), plus(D[i - 1, j], gap_extend))
        I[i, j] = np.maximum(plus(H[i, j - 1], gap_open + gap_extend), plus(I[i, j - 1], gap_extend))
        H[i, j] = np.maximum(np.maximum(D[i, j], I[i, j]), plus(H[i - 1, j - 1], s[i - 1, j - 1]))
    return H, I, D, NEG


def host_bounds(scores, gap_open: int, gap_extend: int, band: int, m: int, n: int):
    """(lo, hi) the host's range check derives for every finite stored value: fits_int16's BANW / BAXT bounds with the largest entry in
    place of match and the smallest in place of mismatch"""
    pos = lambda v: max(v, 0)
    neg = lambda v: min(v, 0)
    top, bottom = int(np.max(scores)), int(np.min(scores))
    o, e = gap_open, gap_extend
    g = min(max(band - 1, 0), max(m, n))
    lo_h = neg(bottom) * min(m, n) + neg(o) + neg(e) * g
    hi_h = pos(top) * min(m, n) + (pos(o) + pos(e)) * (m + n)
    return lo_h + neg(o + e), hi_h + pos(o) + pos(e) * max(m, n)


# the ties-and-zeros fuzz set: two letters, m and n in 0..13, bands 1..5, 40 pairs per band, under four tables
FUZZ_TABLES = [[[0, 0], [0, 0]], [[1, 1], [1, 1]], [[1, 0], [0, 1]], [[2, -3], [1, -1]]]
FUZZ_GAPS = (-3, -1)


def fuzz_code():
    code = np.zeros(256, np.uint8)
    code[66] = 1
    return code


def fuzz_pairs(band: int, banw: bool):
    """the 40 (reference, query) pairs of `band`; banw: lengths redrawn until BANW admits them (|m - n| <= band - 1)"""
    rng = np.random.default_rng(7700 + band + (100 if banw else 0))
    texts = []
    while len(texts) < 40:
        n, m = int(rng.integers(0, 14)), int(rng.integers(0, 14))
        if banw and abs(m - n) >= band:
            continue
        texts.append((rng.integers(65, 67, n).astype(np.uint8).tobytes(), rng.integers(65, 67, m).astype(np.uint8).tobytes()))
    return texts


class SubstOracle:
    def __init__(self, path):
        lib = C.CDLL(path)
        lib.subst_fill.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_int] + [_vp] * 9
        lib.subst_fill.restype = C.c_int
        lib.subst_walk.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_char_p, C.c_char_p,
                                   C.c_char_p]
        lib.subst_walk.restype = C.c_int
        lib.subst_neg_inf.restype = C.c_longlong
        self.lib = lib
        self.neg_inf = lib.subst_neg_inf()

    def align(self, ref: bytes, qry: bytes, scores, code_of, gap_open: int, gap_extend: int, band: int, ext: bool, walk: bool = True,
              raw: bool = False):
        """dict: H, I, D (int32, the exported form), rawH, rawI, rawD (int64, neg_inf for -infinity; only with `raw`), dirH, dirI, dirD
        (uint8), all (m+1) x (n+1); score, end (row, col); lines (ref, rel, qry) as bytes.  ext: BAXT's end cell, else BANW's"""
        n, m = len(ref), len(qry)
        tab = np.ascontiguousarray(scores, np.int8)
        code = np.ascontiguousarray(code_of, np.uint8)
        shape = (m + 1, n + 1)
        H, I, D = (np.zeros(shape, np.int64) for _ in range(3))
        dH, dI, dD = (np.zeros(shape, np.uint8) for _ in range(3))
        sc, er, ec = C.c_int64(), C.c_int32(), C.c_int32()
        rc = self.lib.subst_fill(ref, n, qry, m, tab.ctypes.data, tab.shape[0], code.ctypes.data, gap_open, gap_extend, band, int(ext),
                                 H.ctypes.data, I.ctypes.data, D.ctypes.data, dH.ctypes.data, dI.ctypes.data, dD.ctypes.data,
                                 C.addressof(sc), C.addressof(er), C.addressof(ec))
        assert rc == 0, rc
        eH, eI, eD = exported((H, I, D), self.neg_inf, m, n, band)
        out = {"H": eH, "I": eI, "D": eD, "dirH": dH, "dirI": dI, "dirD": dD, "score": sc.value, "end": (er.value, ec.value)}
        if raw:
            out.update(rawH=H, rawI=I, rawD=D)
        if walk:
            bufs = [C.create_string_buffer(m + n + 2) for _ in range(3)]
            k = self.lib.subst_walk(ref, n, qry, m, band, er.value, ec.value, dH.ctypes.data, dI.ctypes.data, dD.ctypes.data, *bufs)
            assert k >= 0, "the walk left the band"
            out["lines"] = tuple(b.raw[:k] for b in bufs)
        return out

    def result(self, ref: bytes, qry: bytes, scores, code_of, gap_open: int, gap_extend: int, band: int, ext: bool):
        """(score, end row, end column) without the matrices"""
        tab = np.ascontiguousarray(scores, np.int8)
        code = np.ascontiguousarray(code_of, np.uint8)
        sc, er, ec = C.c_int64(), C.c_int32(), C.c_int32()
        rc = self.lib.subst_fill(ref, len(ref), qry, len(qry), tab.ctypes.data, tab.shape[0], code.ctypes.data, gap_open, gap_extend, band,
                                 int(ext), None, None, None, None, None, None, C.addressof(sc), C.addressof(er), C.addressof(ec))
        assert rc == 0, rc
        return sc.value, er.value, ec.value

    def block(self, number: int, ref: bytes, qry: bytes, scores, code_of, gap_open: int, gap_extend: int, band: int, ext: bool) -> bytes:
        """the pair's text block as the output pipeline prints it ("<pair> | <score>" and three lines)"""
        r = self.align(ref, qry, scores, code_of, gap_open, gap_extend, band, ext)
        return b"%d | %d\n" % (number, r["score"]) + b"".join(x + b"\n" for x in r["lines"])


def build(out_dir) -> SubstOracle:
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    so = os.path.join(str(out_dir), "libsubst_oracle.so")
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-o", so, SRC], check=True)
    return SubstOracle(so)
