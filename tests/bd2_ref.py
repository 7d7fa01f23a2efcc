"""What the tests of two-piece band-direction batches (DPX_TWO_PIECE_GAPS, k_bd2_fill) share.  TEST INFRASTRUCTURE ONLY -- never imported
by the product.

* Bd2Oracle: ctypes access to tests/bd2_oracle.c, the int64 band-only oracle of the definition in include/dpx_align.h.  build(dir)
  compiles it with `cc -O2 -shared -fPIC` into `dir`.  expect(): everything a two-piece batch reports for one pair: record, chosen
  score and end cell, traceback lines and the six exported planes, masked behind lastDiag.
* MODES: the eight modes of k_bd2_fill; rescore(): a pair's lines scored under a table and the two pieces."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from bdx_ref import byte_table, cpl  # noqa: F401  (shared helpers, re-exported)
from zext_ref import FIELDS

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "bd2_oracle.c")
_vp = C.c_void_p
BANW, BAXT = 7, 10
NEG_INF = -(2**63) // 4
TWO_PIECE, BAND_DIRS = 0x20, 0x10

# (name, algorithm, table?, zdrop on?, end bonus on?): one per (EXT, TABLE, SCAN) instantiation family of k_bd2_fill
MODES = [("banw_plain", BANW, False, False, False), ("banw_table", BANW, True, False, False), ("baxt_plain", BAXT, False, False, False),
         ("baxt_table", BAXT, True, False, False), ("baxt_bonus", BAXT, False, False, True), ("baxt_drop", BAXT, False, True, True),
         ("baxt_table_bonus", BAXT, True, False, True), ("baxt_table_drop", BAXT, True, True, True)]


def gd(band):
    """steps per 16-byte store of the 8-bit layout (csrc/dpx_banddir2.h)"""
    return 16 // cpl(band)


def chunks(m, n, band):
    return 0 if m <= 0 or n <= 0 else -(-(m + n - 1) // gd(band))


class Bd2Oracle:
    def __init__(self, path):
        lib = C.CDLL(path)
        lib.bd2_fill.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, _vp, C.c_int, _vp] + [C.c_int] * 8 + [_vp] * 8
        lib.bd2_fill.restype = C.c_int
        self.lib = lib

    def expect(self, ref: bytes, qry: bytes, scores, code_of, piece1, piece2, band, ext=True, zdrop=-1, end_bonus=-1, planes=True,
               lines=True, h=False):
        """dict: rec (dpx_extension's fields by name; None for BANW and for BAXT without the scan), score, end (the chosen ones),
        lines (the three lines, or None), dirs (the six planes in selector order, or None), H (int64 scores with h=True; NEG_INF
        where no cell was computed)"""
        n, m = len(ref), len(qry)
        tab = np.ascontiguousarray(scores, np.int8)
        code = np.ascontiguousarray(code_of, np.uint8)
        rec, chosen = np.zeros(8, np.int32), np.zeros(3, np.int32)
        pl = np.zeros((6, m + 1, n + 1), np.uint8) if planes else None
        bufs = [C.create_string_buffer(m + n + 2) for _ in range(3)] if lines else [None] * 3
        k = C.c_int32(0)
        hv = np.zeros((m + 1, n + 1), np.int64) if h else None
        rc = self.lib.bd2_fill(ref, n, qry, m, tab.ctypes.data, tab.shape[0], code.ctypes.data, piece1[0], piece1[1], piece2[0], piece2[1],
                               band, 1 if ext else 0, zdrop, end_bonus, rec.ctypes.data, chosen.ctypes.data,
                               pl.ctypes.data if planes else None, *bufs, C.addressof(k) if lines else None, hv.ctypes.data if h else None)
        assert rc == 0, rc
        assert not lines or k.value >= 0, "the walk left the band"
        r = dict(zip(FIELDS, (int(x) for x in rec))) if ext and (zdrop >= 0 or end_bonus >= 0) else None
        return {"rec": r, "score": int(chosen[0]), "end": (int(chosen[1]), int(chosen[2])),
                "lines": tuple(b.raw[:k.value] for b in bufs) if lines else None, "dirs": tuple(pl) if planes else None,
                "last": int(rec[5]) if ext else m + n, "H": hv}


def build(out_dir) -> Bd2Oracle:
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    so = os.path.join(str(out_dir), "libbd2_oracle.so")
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-o", so, SRC], check=True)
    return Bd2Oracle(so)


def gap(k, piece1, piece2):
    return max(piece1[0] + k * piece1[1], piece2[0] + k * piece2[1])


def rescore(lines, scores, code_of, piece1, piece2):
    """(score, rows, columns) of an alignment given as its three lines: table entries on the columns, g(k) per gap of k columns"""
    lr, _, lq = lines
    total, rows, cols, run, k = 0, 0, 0, None, 0
    for r, q in list(zip(lr, lq)) + [(0, 0)]:
        kind = "I" if q == 95 else "D" if r == 95 else None  # '_' in the query line: the reference byte is inserted
        if kind != run and run is not None:
            total += gap(k, piece1, piece2)
            k = 0
        if kind is None:
            if (r, q) != (0, 0):
                total += int(scores[code_of[r]][code_of[q]])
                rows += 1
                cols += 1
        else:
            k += 1
            rows += kind == "D"
            cols += kind == "I"
        run = kind
    return total, rows, cols
