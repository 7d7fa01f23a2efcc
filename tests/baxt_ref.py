"""ctypes access to the BAXT CPU oracle (tests/baxt_oracle.c).  TEST INFRASTRUCTURE ONLY -- never imported by the product.
build(dir) compiles it with `cc -O2 -shared -fPIC` into `dir` (the test modules' fixtures pass a pytest temporary directory)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "baxt_oracle.c")
_vp = C.c_void_p


def band_mask(m: int, n: int, band: int) -> np.ndarray:
    """(m+1) x (n+1) bool: |i - j| <= band - 1, borders included"""
    i, j = np.mgrid[0:m + 1, 0:n + 1]
    return np.abs(i - j) <= band - 1


def exported(raw, neg_inf: int, m: int, n: int, band: int):
    """H, I, D as dpx_batch_matrix defines them: 0 outside the band, I = D = 0 on in-band borders, in-band -infinity as -32768"""
    inb = band_mask(m, n, band)
    border = np.zeros((m + 1, n + 1), bool)
    border[0, :] = True
    border[:, 0] = True
    out = []
    for k, plane in enumerate(raw):
        v = np.where(plane == neg_inf, -32768, plane)
        v = np.where(inb, v, 0)
        if k:
            v = np.where(border, 0, v)
        out.append(v.astype(np.int32))
    return out


class BaxtOracle:
    def __init__(self, path):
        lib = C.CDLL(path)
        lib.baxt_fill.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [_vp] * 9
        lib.baxt_fill.restype = C.c_int
        lib.baxt_walk.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_char_p, C.c_char_p,
                                  C.c_char_p, _vp, _vp]
        lib.baxt_walk.restype = C.c_int
        lib.baxt_neg_inf.restype = C.c_longlong
        self.lib = lib
        self.neg_inf = lib.baxt_neg_inf()

    def align(self, ref: bytes, qry: bytes, match: int, mismatch: int, gap_open: int, gap_extend: int, band: int, walk: bool = True, raw: bool = True):
        """dict: rawH, rawI, rawD (int64, neg_inf for -infinity; only with `raw`), H, I, D (int32, the exported form), dirH, dirI, dirD
        (uint8), all (m+1) x (n+1); score, end (row, col); lines (ref, rel, qry) as bytes; cells: the walked cells, end cell first"""
        n, m = len(ref), len(qry)
        shape = (m + 1, n + 1)
        H, I, D = (np.zeros(shape, np.int64) for _ in range(3))
        dH, dI, dD = (np.zeros(shape, np.uint8) for _ in range(3))
        sc, er, ec = C.c_int64(), C.c_int32(), C.c_int32()
        rc = self.lib.baxt_fill(ref, n, qry, m, match, mismatch, gap_open, gap_extend, band, H.ctypes.data, I.ctypes.data, D.ctypes.data,
                                dH.ctypes.data, dI.ctypes.data, dD.ctypes.data, C.addressof(sc), C.addressof(er), C.addressof(ec))
        assert rc == 0, rc
        eH, eI, eD = exported((H, I, D), self.neg_inf, m, n, band)
        out = {"H": eH, "I": eI, "D": eD, "dirH": dH, "dirI": dI, "dirD": dD, "score": sc.value, "end": (er.value, ec.value)}
        if raw:
            out.update(rawH=H, rawI=I, rawD=D)
        if walk:
            bufs = [C.create_string_buffer(m + n + 2) for _ in range(3)]
            cells = np.zeros((m + n + 1, 2), np.int32)
            nc = C.c_int32()
            k = self.lib.baxt_walk(ref, n, qry, m, band, er.value, ec.value, dH.ctypes.data, dI.ctypes.data, dD.ctypes.data, *bufs,
                                   cells.ctypes.data, C.addressof(nc))
            assert k >= 0, "the walk left the band"
            out["lines"] = tuple(b.raw[:k] for b in bufs)
            out["cells"] = [tuple(int(x) for x in c) for c in cells[:nc.value]]
        return out

    def result(self, ref: bytes, qry: bytes, w, band: int):
        """(score, end row, end column) without the matrices"""
        sc, er, ec = C.c_int64(), C.c_int32(), C.c_int32()
        rc = self.lib.baxt_fill(ref, len(ref), qry, len(qry), *w, band, None, None, None, None, None, None, C.addressof(sc), C.addressof(er),
                                C.addressof(ec))
        assert rc == 0, rc
        return sc.value, er.value, ec.value

    def block(self, number: int, ref: bytes, qry: bytes, w, band: int) -> bytes:
        """the pair's text block as the output pipeline prints it (ANW's layout: "<pair> | <score>" and three lines)"""
        r = self.align(ref, qry, *w, band, raw=False)
        return b"%d | %d\n" % (number, r["score"]) + b"".join(x + b"\n" for x in r["lines"])


def build(out_dir) -> BaxtOracle:
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    so = os.path.join(str(out_dir), "libbaxt_oracle.so")
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-o", so, SRC], check=True)
    return BaxtOracle(so)
