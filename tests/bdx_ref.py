"""What the tests of dpx_batch_set_direction_scoring (k_bdx_fill) share.  TEST INFRASTRUCTURE ONLY -- never imported by the product.

* BdxOracle: ctypes access to tests/bdx_oracle.c, the band-only oracle (records and the chosen score and end cell of pairs too long for
  the full-matrix oracles).  build(dir) compiles it with `cc -O2 -shared -fPIC` into `dir`.
* expect(): everything a band-direction batch reports for one pair, from tests/zsub_oracle.c (int64 cells, no int16 limit): record,
  chosen score and end cell, traceback lines and the three exported direction planes, masked behind lastDiag.
* MODES: the six modes of k_bdx_fill; the drop sweep of the issue (sweep_cases); rescore(): a pair's lines scored under a table."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

import banw_ref
import zsub_ref
from zext_ref import FIELDS, computed_mask

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "bdx_oracle.c")
_vp = C.c_void_p
BANW, BAXT = 7, 10

# (name, algorithm, table?, zdrop on?, end bonus on?): one per (EXT, TABLE, SCAN) instantiation family of k_bdx_fill
MODES = [("banw_table", BANW, True, False, False), ("baxt_table", BAXT, True, False, False), ("baxt_bonus", BAXT, False, False, True),
         ("baxt_drop", BAXT, False, True, True), ("baxt_table_bonus", BAXT, True, False, True), ("baxt_table_drop", BAXT, True, True, True)]


def cpl(band):
    return 1 if band <= 64 else 2 if band <= 128 else 4 if band <= 256 else 8


class BdxOracle:
    def __init__(self, path):
        lib = C.CDLL(path)
        lib.bdx_fill.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, _vp, C.c_int, _vp] + [C.c_int] * 6 + [_vp] * 2
        lib.bdx_fill.restype = C.c_int
        self.lib = lib

    def fill(self, ref: bytes, qry: bytes, scores, code_of, gap_open, gap_extend, band, ext=True, zdrop=-1, end_bonus=-1):
        """dict: rec (dpx_extension's fields by name; zeros for BANW), score and end (the chosen ones)"""
        tab = np.ascontiguousarray(scores, np.int8)
        code = np.ascontiguousarray(code_of, np.uint8)
        rec, chosen = np.zeros(8, np.int32), np.zeros(3, np.int32)
        rc = self.lib.bdx_fill(ref, len(ref), qry, len(qry), tab.ctypes.data, tab.shape[0], code.ctypes.data, gap_open, gap_extend, band,
                               1 if ext else 0, zdrop, end_bonus, rec.ctypes.data, chosen.ctypes.data)
        assert rc == 0, rc
        return {"rec": dict(zip(FIELDS, (int(x) for x in rec))), "score": int(chosen[0]), "end": (int(chosen[1]), int(chosen[2]))}


def build(out_dir) -> BdxOracle:
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "no C compiler"
    so = os.path.join(str(out_dir), "libbdx_oracle.so")
    subprocess.run([cc, "-O2", "-shared", "-fPIC", "-o", so, SRC], check=True)
    return BdxOracle(so)


def expect(zs: zsub_ref.ZsubOracle, ref: bytes, qry: bytes, scores, code_of, gap_open, gap_extend, band, ext=True, zdrop=-1, end_bonus=-1):
    """dict: rec (None for BANW and for BAXT without the scan), score, end, lines, dirs = the exported (H, I, D) planes: the oracle's
    enum matrices with ANW's borders on the in-band border cells of H, and every plane 0 where i + j > lastDiag"""
    n, m = len(ref), len(qry)
    tab = np.ascontiguousarray(scores, np.int8)
    code = np.ascontiguousarray(code_of, np.uint8)
    shape = (m + 1, n + 1)
    dH, dI, dD = (np.zeros(shape, np.uint8) for _ in range(3))
    last = m + n
    if ext:
        rec, chosen, bc = np.zeros(8, np.int32), np.zeros(3, np.int32), np.zeros(2, np.int32)
        rc = zs.lib.zsub_fill(ref, n, qry, m, tab.ctypes.data, tab.shape[0], code.ctypes.data, gap_open, gap_extend, band, zdrop, end_bonus,
                              None, None, None, dH.ctypes.data, dI.ctypes.data, dD.ctypes.data, rec.ctypes.data, chosen.ctypes.data,
                              bc.ctypes.data)
        assert rc == 0, rc
        r = dict(zip(FIELDS, (int(x) for x in rec)))
        score, end = int(chosen[0]), (int(chosen[1]), int(chosen[2]))
        last = r["lastDiag"]
        if zdrop < 0 and end_bonus < 0:
            r = None
    else:
        sc, er, ec = C.c_int64(), C.c_int32(), C.c_int32()
        zs.lib.subst_fill.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, _vp, C.c_int, _vp, C.c_int, C.c_int, C.c_int, C.c_int] + [_vp] * 9
        zs.lib.subst_fill.restype = C.c_int
        rc = zs.lib.subst_fill(ref, n, qry, m, tab.ctypes.data, tab.shape[0], code.ctypes.data, gap_open, gap_extend, band, 0, None, None, None,
                               dH.ctypes.data, dI.ctypes.data, dD.ctypes.data, C.addressof(sc), C.addressof(er), C.addressof(ec))
        assert rc == 0, rc
        r, score, end = None, int(sc.value), (int(er.value), int(ec.value))
    bufs = [C.create_string_buffer(m + n + 2) for _ in range(3)]
    k = zs.lib.subst_walk(ref, n, qry, m, band, end[0], end[1], dH.ctypes.data, dI.ctypes.data, dD.ctypes.data, *bufs)
    assert k >= 0, "the walk left the band"
    inb = banw_ref.band_mask(m, n, band)
    h = dH.copy()
    h[1:, 0] = np.where(inb[1:, 0], 4, 0)
    h[0, 1:] = np.where(inb[0, 1:], 3, 0)
    h[0, 0] = 0
    keep = computed_mask(m, n, last)
    return {"rec": r, "score": score, "end": end, "lines": tuple(b.raw[:k] for b in bufs),
            "dirs": tuple(np.where(keep, v, 0).astype(np.uint8) for v in (h, dI, dD))}


def byte_table(match, mismatch, used: bytes = b"ACGTN"):
    """(scores, code_of) scoring exactly as byte equality does over the distinct bytes of `used`; every other byte takes code 0"""
    letters = sorted(set(used))
    code = np.zeros(256, np.uint8)
    for k, ch in enumerate(letters):
        code[ch] = k
    scores = np.full((len(letters), len(letters)), mismatch, np.int8)
    np.fill_diagonal(scores, match)
    return scores, code


# ---- the drop sweep: P + "A" * 60 against P + "C" * 60, P a random ACGT prefix of length L; acgtn_table, gaps (-5, -1), E = 5 ----
SWEEP_GAPS, SWEEP_E, SWEEP_Z = zsub_ref.GAPS, 5, (7, 12)
SWEEP_BANDS = {15: 40, 16: 40, 64: 40, 100: 150, 200: 260, 300: 380, 512: 560}  # band: first L


def sweep_pair(rng, L):
    p = rng.integers(0, 4, L).astype(np.uint8)
    p = np.frombuffer(b"ACGT", np.uint8)[p].tobytes()
    return p + b"A" * 60, p + b"C" * 60


def sweep_cases(band):
    """[(L, ref, qry)] for the Gd + 2 consecutive prefix lengths of `band`"""
    gd = 32 // cpl(band)
    rng = np.random.default_rng(9000 + band)
    return [(L,) + sweep_pair(rng, L) for L in range(SWEEP_BANDS[band], SWEEP_BANDS[band] + gd + 2)]


# The sweep's tails of 60 bases end the matrix soon after the drop: from a band of about 114 on the dropping step lies in the fill's TAIL
# phase (interior needs every in-band slot inside the matrix: a <= 2m - B + 1).  So the bands of 100 and up get pairs of the same make
# with tails of B + 70 bases beside the sweep's, whose drops at both Z lie in the interior phase; phase_of() says so from the geometry.
# Equal tails of A against C drop on an even anti-diagonal, the first step of a loop body; a reference tail of G under a query tail of A
# (the table's one asymmetric entry, -1) drops on an odd one, the second step.
INTERIOR_BANDS = (100, 200, 300, 512)


def interior_cases(band):
    """[(L, ref, qry, step)]: four consecutive prefix lengths, each with both kinds of tail (band + 70 bases); step = the step of the
    loop body the pair is meant to drop on, at both Z"""
    rng = np.random.default_rng(9500 + band)
    out = []
    for L in range(SWEEP_BANDS[band], SWEEP_BANDS[band] + 4):
        p = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)].tobytes()
        out.append((L, p + b"A" * (band + 70), p + b"C" * (band + 70), 0))
        out.append((L, p + b"G" * (band + 70), p + b"A" * (band + 70), 1))
    return out


def phase_of(m, n, B, A):
    """("head" | "interior" | "tail", 0 | 1): the phase loop of k_bdx_fill / k_bdir_fill that runs step A (anti-diagonal A + 2) of an
    m x n pair at band B, and whether A is the first or the second step of its loop body -- the kernel's geometry, restated"""
    def interior(A):
        aa = A + 2
        pp = (aa + B - 1) & 1
        ii0 = (aa + pp - (B - 1)) >> 1
        jj0, top = aa - ii0, B - 1 - pp
        return ii0 >= 1 and ii0 + top <= m and jj0 - top >= 1 and jj0 <= n

    NS, A0 = m + n - 1, 0
    assert 0 <= A < NS + (NS & 1)
    while A0 < NS and not (interior(A0) and interior(A0 + 1)):
        if A0 <= A <= A0 + 1:
            return "head", A - A0
        A0 += 2
    while A0 + 2 < NS and interior(A0 + 1):
        if A0 <= A <= A0 + 1:
            return "interior", A - A0
        A0 += 2
    return "tail", A & 1


def sweep_last_diag(band, L, Z):
    """the issue's statement of where the sweep's pairs drop"""
    if Z == 7:
        return 2 * L + 6
    return 2 * L + (19 if band == 15 else 20 if band == 16 else 63)


def rescore(lines, scores, code_of, gap_open, gap_extend):
    """(score, rows, columns) of an alignment given as its three lines: table entries on the columns, gap_open + k * gap_extend per gap"""
    lr, _, lq = lines
    total, rows, cols, run = 0, 0, 0, None
    for r, q in zip(lr, lq):
        kind = "I" if q == 95 else "D" if r == 95 else None  # '_' in the query line: the reference byte is inserted
        if kind is None:
            total += int(scores[code_of[r]][code_of[q]])
            rows += 1
            cols += 1
        else:
            total += gap_extend + (gap_open if kind != run else 0)
            rows += kind == "D"
            cols += kind == "I"
        run = kind
    return total, rows, cols
