"""ctypes access to the ASG CPU oracle (tests/asg_oracle.c).  TEST INFRASTRUCTURE ONLY -- never imported by the product.
build(dir) compiles it with `cc -O2 -shared -fPIC` into `dir` (the test modules' fixtures pass a pytest temporary directory)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "asg_oracle.c")
_vp = C.c_void_p


class AsgOracle:
    def __init__(self, path):
        lib = C.CDLL(path)
        lib.asg_fill.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int] + [_vp] * 9
        lib.asg_fill.restype = C.c_int
        lib.asg_walk.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int,
                                 C.c_char_p, C.c_char_p, C.c_char_p]
        lib.asg_walk.restype = C.c_int
        self.lib = lib

    def align(self, ref: bytes, qry: bytes, match: int, mismatch: int, gap_open: int, gap_extend: int, matrices: bool = True):
        """dict: H, I, D (int32), dirH, dirI, dirD (uint8), all (m+1) x (n+1); score, end (row, col); lines (ref, rel, qry) as bytes"""
        n, m = len(ref), len(qry)
        shape = (m + 1, n + 1)
        H, I, D = (np.zeros(shape, np.int32) for _ in range(3)) if matrices else (None, None, None)
        dH, dI, dD = (np.zeros(shape, np.uint8) for _ in range(3))
        sc, er, ec = C.c_int32(), C.c_int32(), C.c_int32()
        ptr = lambda a: a.ctypes.data if a is not None else None
        rc = self.lib.asg_fill(ref, n, qry, m, match, mismatch, gap_open, gap_extend, ptr(H), ptr(I), ptr(D),
                               dH.ctypes.data, dI.ctypes.data, dD.ctypes.data, C.addressof(sc), C.addressof(er), C.addressof(ec))
        assert rc == 0
        bufs = [C.create_string_buffer(m + n + 2) for _ in range(3)]
        k = self.lib.asg_walk(ref, n, qry, m, dH.ctypes.data, dI.ctypes.data, dD.ctypes.data, er.value, ec.value, *bufs)
        return {"H": H, "I": I, "D": D, "dirH": dH, "dirI": dI, "dirD": dD, "score": sc.value, "end": (er.value, ec.value),
                "lines": tuple(b.raw[:k] for b in bufs)}

    def block(self, number: int, ref: bytes, qry: bytes, w) -> bytes:
        """the pair's text block as the output pipeline prints it ("<pair> | <score>" and three lines, whatever the score's sign)"""
        r = self.align(ref, qry, *w, matrices=False)
        return b"%d | %d\n" % (number, r["score"]) + b"".join(x + b"\n" for x in r["lines"])


def build(out_dir) -> AsgOracle:
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    so = os.path.join(str(out_dir), "libasg_oracle.so")
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-o", so, SRC], check=True)
    return AsgOracle(so)
