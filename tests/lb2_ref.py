"""What the tests of two-piece local band-direction batches (DPX_LOCAL_TWO_PIECE_GAPS, k_lb2_fill) share.  TEST INFRASTRUCTURE ONLY --
never imported by the product.

* Lb2Oracle: ctypes access to tests/lb2_oracle.c, the int64 band-only oracle of the definition in include/dpx_align.h.  build(dir)
  compiles it with `cc -O2 -shared -fPIC` into `dir`.  align(): everything such a batch reports for one pair: score, end cell, the three
  lines, the six exported planes and optionally H.
* rescore(): a pair's lines scored under match / mismatch or a table and the two pieces; block(): the pair's text block."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "lb2_oracle.c")
BASW = 5
LOCAL_BAND_DIRS, LOCAL_TWO_PIECE = 0x40, 0x80
_vp = C.c_void_p


class Lb2Oracle:
    def __init__(self, path):
        lib = C.CDLL(path)
        lib.lb2_align.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, _vp, C.c_int, _vp] + [C.c_int] * 7 + [_vp] * 3 + [C.c_char_p] * 3 + [_vp] * 2
        lib.lb2_align.restype = C.c_int
        self.lib = lib

    def align(self, ref: bytes, qry: bytes, scoring, piece1, piece2, band: int, planes: bool = False, h: bool = False):
        """scoring = (match, mismatch), or (scores, code_of) for a table.  dict: score, end (row, col), lines (ref, rel, qry) as bytes,
        dirs (the six planes in selector order, uint8 (m+1) x (n+1); None without planes=True) and H (int64; None without h=True)"""
        n, m = len(ref), len(qry)
        table = not np.isscalar(scoring[0])
        if table:
            tab, code = np.ascontiguousarray(scoring[0], np.int8), np.ascontiguousarray(scoring[1], np.uint8)
            assert tab.ndim == 2 and tab.shape[0] == tab.shape[1] and code.shape == (256,)
            targs = (tab.ctypes.data, tab.shape[0], code.ctypes.data, 0, 0)
        else:
            targs = (None, 0, None, int(scoring[0]), int(scoring[1]))
        sc, er, ec = C.c_int64(), C.c_int32(), C.c_int32()
        bufs = [C.create_string_buffer(m + n + 2) for _ in range(3)]
        pl = np.zeros((6, m + 1, n + 1), np.uint8) if planes else None
        hv = np.zeros((m + 1, n + 1), np.int64) if h else None
        k = self.lib.lb2_align(ref, n, qry, m, *targs, piece1[0], piece1[1], piece2[0], piece2[1], band, C.addressof(sc), C.addressof(er),
                               C.addressof(ec), *bufs, pl.ctypes.data if planes else None, hv.ctypes.data if h else None)
        assert k >= 0, k
        return {"score": sc.value, "end": (er.value, ec.value), "lines": tuple(b.raw[:k] for b in bufs), "dirs": tuple(pl) if planes else None,
                "H": hv}

    def block(self, number: int, ref: bytes, qry: bytes, scoring, piece1, piece2, band: int) -> bytes:
        """the pair's text block as the output pipeline prints it (LSW's layout: "<pair> | <score>" and three lines)"""
        r = self.align(ref, qry, scoring, piece1, piece2, band)
        return b"%d | %d\n" % (number, r["score"]) + b"".join(x + b"\n" for x in r["lines"])


def build(out_dir) -> Lb2Oracle:
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    so = os.path.join(str(out_dir), "liblb2_oracle.so")
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-o", so, SRC], check=True)
    return Lb2Oracle(so)


def gap(k, piece1, piece2):
    return max(piece1[0] + k * piece1[1], piece2[0] + k * piece2[1])


def rescore(lines, scoring, piece1, piece2):
    """(score, rows, columns) of an alignment given as its three lines: the diagonal term on the columns, g(k) per gap of k columns"""
    lr, _, lq = lines
    table = not np.isscalar(scoring[0])
    total, rows, cols, run, k = 0, 0, 0, None, 0
    for r, q in list(zip(lr, lq)) + [(0, 0)]:
        kind = "I" if q == 95 else "D" if r == 95 else None  # '_' in the query line: the reference byte is inserted
        if kind != run and run is not None:
            total += gap(k, piece1, piece2)
            k = 0
        if kind is None:
            if (r, q) != (0, 0):
                total += int(scoring[0][scoring[1][r]][scoring[1][q]]) if table else (scoring[0] if r == q else scoring[1])
                rows += 1
                cols += 1
        else:
            k += 1
            rows += kind == "D"
            cols += kind == "I"
        run = kind
    return total, rows, cols


def piece2_on_path(r):
    """does the walked path of align(planes=True)'s result hold a gap move of piece 2?  The path's cells are found from the end cell
    and the lines; H_PIECE == 2 on a cell of the path whose H move is a gap"""
    (i, j), (lr, _, lq) = r["end"], r["lines"]
    piece = r["dirs"][5]
    state = None
    for a, b in zip(reversed(lr), reversed(lq)):
        kind = "I" if b == 95 else "D" if a == 95 else None
        if kind is not None and kind != state and piece[i, j] == 2:  # (the cell where the walk entered the gap from SCORING)
            return True
        state = kind
        if kind is None:
            i, j = i - 1, j - 1
        elif kind == "I":
            j -= 1
        else:
            i -= 1
    return False
