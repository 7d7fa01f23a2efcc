"""ctypes access to the BASW CPU oracle (tests/basw_oracle.c).  TEST INFRASTRUCTURE ONLY -- never imported by the product.
build(dir) compiles it with `cc -O2 -shared -fPIC` into `dir` (the test modules' fixtures pass a pytest temporary directory)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "basw_oracle.c")
_vp = C.c_void_p


class BaswOracle:
    def __init__(self, path):
        lib = C.CDLL(path)
        lib.basw_fill.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [_vp] * 9
        lib.basw_fill.restype = C.c_int
        lib.basw_walk.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_int, C.c_int,
                                  C.c_char_p, C.c_char_p, C.c_char_p]
        lib.basw_walk.restype = C.c_int
        self.lib = lib

    def align(self, ref: bytes, qry: bytes, match: int, mismatch: int, gap_open: int, gap_extend: int, band: int, walk: bool = True):
        """dict: H, I, D (int32), dirH, dirI, dirD (uint8), all (m+1) x (n+1); score, end (row, col); lines (ref, rel, qry) as bytes"""
        n, m = len(ref), len(qry)
        shape = (m + 1, n + 1)
        H, I, D = (np.zeros(shape, np.int32) for _ in range(3))
        dH, dI, dD = (np.zeros(shape, np.uint8) for _ in range(3))
        sc, er, ec = C.c_int32(), C.c_int32(), C.c_int32()
        rc = self.lib.basw_fill(ref, n, qry, m, match, mismatch, gap_open, gap_extend, band, H.ctypes.data, I.ctypes.data, D.ctypes.data,
                                dH.ctypes.data, dI.ctypes.data, dD.ctypes.data, C.addressof(sc), C.addressof(er), C.addressof(ec))
        assert rc == 0
        out = {"H": H, "I": I, "D": D, "dirH": dH, "dirI": dI, "dirD": dD, "score": sc.value, "end": (er.value, ec.value)}
        if walk:
            bufs = [C.create_string_buffer(m + n + 2) for _ in range(3)]
            k = self.lib.basw_walk(ref, n, qry, m, band, H.ctypes.data, dH.ctypes.data, dI.ctypes.data, dD.ctypes.data, er.value, ec.value,
                                   *bufs)
            assert k >= 0, "the walk left the band"
            out["lines"] = tuple(b.raw[:k] for b in bufs)
        return out

    def score(self, ref: bytes, qry: bytes, w, band: int) -> int:
        n, m = len(ref), len(qry)
        sc, er, ec = C.c_int32(), C.c_int32(), C.c_int32()
        rc = self.lib.basw_fill(ref, n, qry, m, *w, band, None, None, None, None, None, None, C.addressof(sc), C.addressof(er),
                                C.addressof(ec))
        assert rc == 0
        return sc.value

    def block(self, number: int, ref: bytes, qry: bytes, w, band: int) -> bytes:
        """the pair's text block as the output pipeline prints it (LSW's layout: "<pair> | <score>" and three lines)"""
        r = self.align(ref, qry, *w, band)
        return b"%d | %d\n" % (number, r["score"]) + b"".join(x + b"\n" for x in r["lines"])


def build(out_dir) -> BaswOracle:
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    so = os.path.join(str(out_dir), "libbasw_oracle.so")
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-o", so, SRC], check=True)
    return BaswOracle(so)
