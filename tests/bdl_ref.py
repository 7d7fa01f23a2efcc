"""ctypes access to the band-only BSW / BASW CPU oracle (tests/bdl_oracle.c).  TEST INFRASTRUCTURE ONLY -- never imported by the product.
build(dir) compiles it with `cc -O2 -shared -fPIC` into `dir` (the test modules' fixtures pass a pytest temporary directory)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "bdl_oracle.c")
BSW, BASW = 3, 5
_vp = C.c_void_p


def weights(algo, w):
    """(match, mismatch, gapOpen, gapExtend) of a batch from a weight set of either length: BSW takes the first three"""
    return tuple(w[:3]) + ((w[3],) if algo == BASW else (0,))


class BdlOracle:
    def __init__(self, path):
        lib = C.CDLL(path)
        lib.bdl_align.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int] + [C.c_int] * 6 + [_vp] * 3 + [C.c_char_p] * 3 + [_vp] * 3
        lib.bdl_align.restype = C.c_int
        self.lib = lib

    def align(self, algo: int, ref: bytes, qry: bytes, w, band: int, planes: bool = False):
        """dict: score, end (row, col), lines (ref, rel, qry) as bytes and, planes=True, dirH / dirI / dirD (uint8, (m+1) x (n+1))"""
        n, m = len(ref), len(qry)
        match, mismatch, o, e = weights(algo, w)
        sc, er, ec = C.c_int64(), C.c_int32(), C.c_int32()
        bufs = [C.create_string_buffer(m + n + 2) for _ in range(3)]
        dirs = [np.zeros((m + 1, n + 1), np.uint8) for _ in range(3)] if planes else [None] * 3
        k = self.lib.bdl_align(ref, n, qry, m, int(algo == BASW), match, mismatch, o, e, band, C.addressof(sc), C.addressof(er), C.addressof(ec),
                               *bufs, *[d.ctypes.data if d is not None else None for d in dirs])
        assert k >= 0, k
        out = {"score": sc.value, "end": (er.value, ec.value), "lines": tuple(b.raw[:k] for b in bufs)}
        if planes:
            out.update(dirH=dirs[0], dirI=dirs[1], dirD=dirs[2])
        return out

    def block(self, number: int, algo: int, ref: bytes, qry: bytes, w, band: int) -> bytes:
        """the pair's text block as the output pipeline prints it (LSW's layout: "<pair> | <score>" and three lines)"""
        r = self.align(algo, ref, qry, w, band)
        return b"%d | %d\n" % (number, r["score"]) + b"".join(x + b"\n" for x in r["lines"])


def build(out_dir) -> BdlOracle:
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    so = os.path.join(str(out_dir), "libbdl_oracle.so")
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-o", so, SRC], check=True)
    return BdlOracle(so)
