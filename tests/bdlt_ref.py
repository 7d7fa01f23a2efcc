"""ctypes access to the band-only BSW / BASW CPU oracle under a substitution table (tests/bdlt_oracle.c), and the tables the bdlt tests
share.  TEST INFRASTRUCTURE ONLY -- never imported by the product.  build(dir) compiles the oracle with `cc -O2 -shared -fPIC` into `dir`
(the test modules' fixtures pass a pytest temporary directory)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "bdlt_oracle.c")
BSW, BASW = 3, 5
_vp = C.c_void_p


def gaps(algo, g):
    """(gapOpen, gapExtend) of a batch from a pair of gap weights: BSW takes the first as its one gap weight"""
    return (g[0], g[1] if algo == BASW else 0)


def identity_table(match, mismatch, letters: bytes):
    """a table equivalent to match / mismatch over texts made of `letters` (at most 31): every letter its own code, every other byte the
    last code, which no text uses"""
    assert len(set(letters)) == len(letters) <= 31
    k = len(letters) + 1
    tab = np.full((k, k), mismatch, np.int8)
    np.fill_diagonal(tab, match)
    code = np.full(256, k - 1, np.uint8)
    for c, x in enumerate(letters):
        code[x] = c
    return tab, code


def dna_table():
    """5 x 5 over ACGTN: match 2, transition -1, transversion -3, N against anything (N included) -1; lower case folded, every other
    byte is N"""
    tab = np.full((5, 5), -3, np.int8)
    np.fill_diagonal(tab, 2)
    tab[0, 2] = tab[2, 0] = tab[1, 3] = tab[3, 1] = -1
    tab[4, :] = tab[:, 4] = -1
    code = np.full(256, 4, np.uint8)
    for c, x in enumerate(b"ACGT"):
        code[x] = code[x + 32] = c
    return tab, code


def random_table(seed, symmetric=False, alphabet=32):
    """a random int8 table over `alphabet` codes and a map of all 256 bytes onto them (bytes >= 128 included); the asymmetric one holds
    -128 and 127.  Positive on the diagonal more often than not, so that local alignments exist."""
    rng = np.random.default_rng(seed)
    tab = rng.integers(-12, 5, (alphabet, alphabet)).astype(np.int8)
    tab[np.arange(alphabet), np.arange(alphabet)] = rng.integers(1, 12, alphabet)
    if symmetric:
        tab = np.minimum(tab, tab.T)
    else:
        tab[3, 5], tab[5, 3], tab[7, 7] = -128, 127, 127
    code = rng.integers(0, alphabet, 256).astype(np.uint8)
    code[:alphabet] = np.arange(alphabet)  # every code is some byte's
    return np.ascontiguousarray(tab), code


class BdltOracle:
    def __init__(self, path):
        lib = C.CDLL(path)
        lib.bdlt_align.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_int, _vp, C.c_int, _vp] + [C.c_int] * 3 + [_vp] * 3 + [C.c_char_p] * 3 + [_vp] * 3
        lib.bdlt_align.restype = C.c_int
        self.lib = lib

    def align(self, algo: int, ref: bytes, qry: bytes, table, g, band: int, planes: bool = False):
        """dict: score, end (row, col), lines (ref, rel, qry) as bytes and, planes=True, dirH / dirI / dirD (uint8, (m+1) x (n+1)).
        table = (scores, code_of); g = (gapOpen, gapExtend) as gaps() gives them"""
        n, m = len(ref), len(qry)
        tab, code = np.ascontiguousarray(table[0], np.int8), np.ascontiguousarray(table[1], np.uint8)
        assert tab.ndim == 2 and tab.shape[0] == tab.shape[1] and code.shape == (256,)
        sc, er, ec = C.c_int64(), C.c_int32(), C.c_int32()
        bufs = [C.create_string_buffer(m + n + 2) for _ in range(3)]
        dirs = [np.zeros((m + 1, n + 1), np.uint8) for _ in range(3)] if planes else [None] * 3
        k = self.lib.bdlt_align(ref, n, qry, m, int(algo == BASW), tab.ctypes.data, tab.shape[0], code.ctypes.data, g[0], g[1], band,
                                C.addressof(sc), C.addressof(er), C.addressof(ec), *bufs, *[d.ctypes.data if d is not None else None for d in dirs])
        assert k >= 0, k
        out = {"score": sc.value, "end": (er.value, ec.value), "lines": tuple(b.raw[:k] for b in bufs)}
        if planes:
            out.update(dirH=dirs[0], dirI=dirs[1], dirD=dirs[2])
        return out

    def block(self, number: int, algo: int, ref: bytes, qry: bytes, table, g, band: int) -> bytes:
        """the pair's text block as the output pipeline prints it (LSW's layout: "<pair> | <score>" and three lines)"""
        r = self.align(algo, ref, qry, table, g, band)
        return b"%d | %d\n" % (number, r["score"]) + b"".join(x + b"\n" for x in r["lines"])


def build(out_dir) -> BdltOracle:
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    so = os.path.join(str(out_dir), "libbdlt_oracle.so")
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-o", so, SRC], check=True)
    return BdltOracle(so)
