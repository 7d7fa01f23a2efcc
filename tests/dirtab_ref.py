"""ctypes access to the CPU oracle of ANW / ASW / ASG under a substitution table (tests/dirtab_oracle.c), plus an independent NumPy
fill.  TEST INFRASTRUCTURE ONLY -- never imported by the product.  build(dir) compiles the oracle with `cc -O2 -shared -fPIC` into
`dir` (the test modules' fixtures pass a pytest temporary directory)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "dirtab_oracle.c")
_vp = C.c_void_p
KINDS = {"ANW": 0, "ASW": 1, "ASG": 2}


def random_table(rng, alphabet: int, lo: int = -6, hi: int = 7):
    """an asymmetric int8 table (a transposed lookup gives other scores) and a map that sends every byte to some code"""
    scores = rng.integers(lo, hi, (alphabet, alphabet)).astype(np.int8)
    if alphabet > 1 and np.array_equal(scores, scores.T):
        scores[0, 1] = scores[1, 0] + 1
    code = rng.integers(0, alphabet, 256).astype(np.uint8)
    return scores, code


def numpy_result(kind: str, ref: bytes, qry: bytes, scores, code_of, gap_open: int, gap_extend: int):
    """(score, (end row, end column)) from H filled anti-diagonal by anti-diagonal with array operations (the oracle goes row by row):
    an independent second implementation of the definition"""
    NEG = -(1 << 40)
    n, m = len(ref), len(qry)
    code = np.asarray(code_of, np.int64)
    rc, qc = code[np.frombuffer(ref, np.uint8)], code[np.frombuffer(qry, np.uint8)]
    s = np.asarray(scores, np.int64)[rc[None, :], qc[:, None]]  # (m, n): row of the table = reference code
    H = np.zeros((m + 1, n + 1), np.int64)
    I, D = (np.full((m + 1, n + 1), NEG, np.int64) for _ in range(2))
    if kind != "ASW":
        H[1:, 0] = gap_open + np.arange(1, m + 1) * gap_extend
    if kind == "ANW":
        H[0, 1:] = gap_open + np.arange(1, n + 1) * gap_extend
    for a in range(2, m + n + 1):
        i = np.arange(max(1, a - n), min(m, a - 1) + 1)
        j = a - i
        D[i, j] = np.maximum(H[i - 1, j] + gap_open + gap_extend, D[i - 1, j] + gap_extend)
        I[i, j] = np.maximum(H[i, j - 1] + gap_open + gap_extend, I[i, j - 1] + gap_extend)
        h = np.maximum(np.maximum(D[i, j], I[i, j]), H[i - 1, j - 1] + s[i - 1, j - 1])
        H[i, j] = np.maximum(h, 0) if kind == "ASW" else h
    if kind == "ANW":
        return int(H[m, n]), (m, n)
    if kind == "ASG":
        j = int(np.argmax(H[m]))  # the first maximum
        return int(H[m, j]), (m, j)
    top = int(H.max())
    if top <= 0:
        return 0, (0, 0)
    k = int(np.argmax(H))  # the first in row-major order
    return top, (k // (n + 1), k % (n + 1))


class DirtabOracle:
    def __init__(self, path):
        lib = C.CDLL(path)
        lib.dirtab_fill.argtypes = [C.c_int, C.c_char_p, C.c_int, C.c_char_p, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int] + [_vp] * 6
        lib.dirtab_fill.restype = C.c_int
        lib.dirtab_walk.argtypes = [C.c_int, C.c_char_p, C.c_int, C.c_char_p, C.c_int, _vp, _vp, _vp, C.c_int, C.c_int,
                                    C.c_char_p, C.c_char_p, C.c_char_p]
        lib.dirtab_walk.restype = C.c_int
        self.lib = lib

    def align(self, kind: str, ref: bytes, qry: bytes, scores, code_of, gap_open: int, gap_extend: int):
        """dict: dirH, dirI, dirD (uint8, (m+1) x (n+1), the enums dpx_batch_directions exports); score, end (row, col); lines (ref, rel,
        qry) as bytes"""
        n, m = len(ref), len(qry)
        tab = np.ascontiguousarray(scores, np.int8)
        code = np.ascontiguousarray(code_of, np.uint8)
        assert tab.ndim == 2 and tab.shape[0] == tab.shape[1] and code.shape == (256,)
        dH, dI, dD = (np.zeros((m + 1, n + 1), np.uint8) for _ in range(3))
        sc, er, ec = C.c_int64(), C.c_int32(), C.c_int32()
        k = KINDS[kind]
        rc = self.lib.dirtab_fill(k, ref, n, qry, m, tab.ctypes.data, tab.shape[0], code.ctypes.data, gap_open, gap_extend,
                                  dH.ctypes.data, dI.ctypes.data, dD.ctypes.data, C.addressof(sc), C.addressof(er), C.addressof(ec))
        assert rc == 0, rc
        bufs = [C.create_string_buffer(m + n + 2) for _ in range(3)]
        ln = self.lib.dirtab_walk(k, ref, n, qry, m, dH.ctypes.data, dI.ctypes.data, dD.ctypes.data, er.value, ec.value, *bufs)
        assert ln >= 0, "the walk met a cell without a move"
        return {"dirH": dH, "dirI": dI, "dirD": dD, "score": sc.value, "end": (er.value, ec.value), "lines": tuple(b.raw[:ln] for b in bufs)}

    def block(self, number: int, kind: str, ref: bytes, qry: bytes, scores, code_of, gap_open: int, gap_extend: int) -> bytes:
        """the pair's text block as the output pipeline prints it ("<pair> | <score>" and three lines)"""
        r = self.align(kind, ref, qry, scores, code_of, gap_open, gap_extend)
        return b"%d | %d\n" % (number, r["score"]) + b"".join(x + b"\n" for x in r["lines"])


def build(out_dir) -> DirtabOracle:
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    so = os.path.join(str(out_dir), "libdirtab_oracle.so")
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-o", so, SRC], check=True)
    return DirtabOracle(so)
