"""Pairs whose maximal score is placed, cell by cell, where the start-cell keys of k_banded_fill, k_banded_fill_pk and k_linear_fill_pk
must choose between equal maxima (tests/test_gpu_start_ties.py runs them on the GPU; tests/test_tie_cases.py asserts on the oracle alone
that they are what they claim).  TEST INFRASTRUCTURE ONLY -- never imported by the product.

Construction: a motif is a prefix of the pattern `abbabaabba` over a letter pair of its own (AC, GT, BD, EF, HI, JK); the query's filler
is `x`, the reference's `y`, and no letter of one alphabet occurs in another.  A motif of length L that ends on query row r and on
reference column c makes H[r][c] = match * L, occurrences of different motifs never combine, and two cells are kept anti-ordered (or
far apart) so that no path chains them: the tied cells are exactly the placed ones.  Single letters (L = 1) place ties on adjacent
rows, on row 1 and on column 1.

Expectations come from oracle_py.lsw alone (band= for BSW): score, end cell and the three traceback lines, computed once per key."""
import numpy as np

import oracle_py as O
from score_only_cases import shared, tie_texts

W = (3, -1, -2)
PATTERN = "abbabaabba"
LETTERS = (b"AC", b"GT", b"BD", b"EF", b"HI", b"JK")
P, Q = b"ACCACAACCA", b"GTTGTGGTTG"


def motif(kind, L=10):
    a, b = LETTERS[kind][0:1], LETTERS[kind][1:2]
    return b"".join(a if ch == "a" else b for ch in PATTERN[:L])


assert motif(0) == P and motif(1) == Q and len(PATTERN) == 10


def place(size, filler, items):
    """a text of `size` fillers with every (kind, L, end) motif written so that its last letter is character number `end` (1-based)"""
    out = bytearray(filler * size)
    used = np.zeros(size, bool)
    for kind, L, end in items:
        assert L <= end <= size and not used[end - L:end].any(), (size, items)
        out[end - L:end] = motif(kind, L)
        used[end - L:end] = True
    return bytes(out)


def pair(m, n, cells=(), qry=(), ref=(), shift=0):
    """(reference, query): every (kind, L, row, column) of `cells` places its motif in both texts; `qry` / `ref` add (kind, L, end)
    occurrences to one text alone (a second row or column of a motif that `cells` placed).  `shift` moves everything down its diagonal,
    so that the pairs of one list, which share a construction, differ in their answers"""
    q = [(k, L, r + shift) for k, L, r, _ in cells] + [(k, L, e + shift) for k, L, e in qry]
    r = [(k, L, c + shift) for k, L, _, c in cells] + [(k, L, e + shift) for k, L, e in ref]
    return place(n, b"y", r), place(m, b"x", q)


# ---------------------------------------------------------------------------------------------- geometry (csrc/dpx_layout.h)
def band_cpl(B):
    c = (B + 63) // 64
    return 1 if c <= 1 else 2 if c <= 2 else 4 if c <= 4 else 8   # dpx_band_cpl


def band_geo(i, j, B):
    """step, diagonal, slot, lane, cell in lane and store group of in-band cell (i, j)"""
    C = band_cpl(B)
    u = i - j + B - 1
    assert 0 <= u <= 2 * B - 2, (i, j, B)
    s = u >> 1
    return {"A": i + j - 2, "u": u, "slot": s, "lane": s // C, "cell": s % C, "group": (i + j - 2) // max(1, 8 // C)}


def band_phases(m, n, B):
    """(first interior step, first tail step) of the kernels' step loop: head, interior and tail run whole trips of GG steps"""
    C = band_cpl(B)
    GG = max(2, max(1, 8 // C))
    NS = m + n - 1

    def interior(A):
        aa = A + 2
        pp = (aa + B - 1) & 1
        i0 = (aa + pp - (B - 1)) >> 1
        j0, top = aa - i0, B - 1 - pp
        return i0 >= 1 and i0 + top <= m and j0 - top >= 1 and j0 <= n

    A0 = 0
    while A0 < NS and not (interior(A0) and interior(A0 + GG - 1)):
        A0 += GG
    head_end = A0
    while A0 + GG <= NS and interior(A0 + GG - 1):
        A0 += GG
    return head_end, A0


def stripe_geo(i, j, n, R):
    """stripe, lane, row in lane and wave step of cell (i, j) of the wavefront-tiled layout"""
    s = 64 * R
    k, lane = (i - 1) // s, ((i - 1) % s) // R
    return {"stripe": k, "lane": lane, "row": (i - 1) % R, "T": k * n + (j - 1) + lane}


# ---------------------------------------------------------------------------------------------- a. the band cases
BANDS = (17, 64, 65, 128, 129, 256, 257, 512)   # 1, 1, 2, 2, 4, 4, 8 and 8 cells per lane, odd and even
BAND_CLASSES = ("B1", "B2", "B3", "B4a", "B4b", "B5", "B6a", "B6b", "B7h", "B7t", "B7l", "B8", "B9")
BAND_RULES = ("earliest step, then smallest row", "column-major first", "last maximum", "first maximum ignoring the band")
# what a band's geometry does not allow: {band: {class or rule: reason}}
_ONE_CELL = "one cell per lane: a lane holds one slot"
NO_SUCH_BAND_CASE = {17: {"B3": _ONE_CELL}, 64: {"B3": _ONE_CELL}}


MATRIX_PAIRS = (0, 9)   # the pairs of every band whose whole matrix the GPU test compares (the other expectations keep no H)


def band_shape(B):
    return B + 120, B + 120


def band_texts(B):
    """[(name, (reference, query))], every pair of shape band_shape(B); the names only label failure messages -- the classes a pair
    holds are found by band_classes() from the oracle's H"""
    m, n = band_shape(B)
    d, C = B - 1, band_cpl(B)
    w = min(B - 3, 60)
    L, g = (10, 12) if B >= 64 else (3, 5)   # the short motif where three occurrences or a phase of 16 steps leave no room for ten letters
    odd = d & 1
    c3 = 28 + d - (d // (2 * C)) * 2 * C     # the single letters of `adjacent rows` start on cell 0 of a lane
    head = [(0, 10, 11, 25), (1, 10, 25, 12)] if B >= 64 else [(0, 3, 3, 8), (1, 3, 8, 4)]
    tail = [(0, 10, m - 16, n - 2), (1, 10, m - 3, n - 16)] if B >= 64 else [(0, 3, m - 8, n - 3), (1, 3, m - 2, n - 8)]
    low = (1, 10, 42 + d, 42) if d >= 22 else (1, 10, 18 + 2 * d, 18 + d)   # on the lower edge, left of the upper edge's motif
    cases = [
        ("two lanes, first on the later step", pair(m, n, [(0, 10, 30, 30 + w), (1, 10, 42, 30)])),
        ("one diagonal, two steps", pair(m, n, [(0, 10, 30, 30), (1, 10, 70, 70)], shift=3)),
        ("adjacent rows, first on the later step", pair(m, n, [(0, 1, 30, c3 + 2), (1, 1, 31, c3)], shift=7)),
        ("one anti-diagonal, two slots", pair(m, n, [(0, 10, 30, 42), (1, 10, 42, 30)], shift=12)),
        ("the two diagonals of one slot", pair(m, n, [(0, 10, 30, 30 + odd), (1, 10, 71, 70 + odd)], shift=1)),
        ("one row, two columns", pair(m, n, [(0, 10, 30, 30)], ref=[(0, 10, 44)], shift=16)),
        ("two lanes, first on the earlier step", pair(m, n, [(0, 10, 30, 41), (1, 10, 44, 30)], shift=5)),
        ("one column, two rows", pair(m, n, [(0, 10, 30, 37)], qry=[(0, 10, 44)], shift=21)),
        ("head phase", pair(m, n, head)),
        ("out of band at a smaller row", pair(m, n, [(0, 10, 12, B + 30), (1, 10, B + 50, B + 62), (2, 10, B + 62, B + 50)])),
        ("tail phase", pair(m, n, tail)),
        ("three lanes", pair(m, n, [(0, L, 30, 30 + 2 * g), (1, L, 30 + g, 29 + g), (2, L, 30 + 2 * g, 29)], shift=9)),
        ("last anti-diagonal", pair(m, n, [(0, 10, m, n)], qry=[(0, 10, m - 14)])),
        ("both edges of the band", pair(m, n, [(0, 10, 30, 30 + d), low], shift=2)),
        ("control: unique maximum", pair(m, n, [(0, 10, 30, 30), (1, 5, 60, 50)], shift=14)),
        ("control: score 0", pair(m, n)),
        ("control: unique maximum on the band's edge", pair(m, n, [(0, 10, 30 + d, 30)], shift=6)),
        ("one anti-diagonal, three lanes", pair(m, n, [(0, L, 30, 30 + 2 * g), (1, L, 30 + g, 30 + g), (2, L, 30 + 2 * g, 30)], shift=18)),
    ]
    assert len(cases) % 2 == 0 and all(len(r) == n and len(q) == m for _, (r, q) in cases)
    return cases


def tied_cells(H, B=0):
    """the cells that hold the maximum of H, in row-major order (inside the band when B > 0)"""
    m, n = H.shape[0] - 1, H.shape[1] - 1
    Hb = H
    if B > 0:
        i, j = np.indices(H.shape)
        Hb = np.where(np.abs(i - j) <= B - 1, H, 0)
    top = int(Hb[1:, 1:].max()) if m and n else 0
    if top <= 0:
        return 0, []
    return top, [(int(i), int(j)) for i, j in np.argwhere(Hb == top) if i >= 1 and j >= 1]


def band_classes(cells, B, m, n, free=None):
    """the classes B1 .. B9 that the tied in-band `cells` (row-major order) hold.  `free`: (end cell, tied cells) of the unbanded oracle"""
    out = set()
    if len(cells) < 2:
        return out
    geo = [band_geo(i, j, B) for i, j in cells]
    head_end, tail_start = band_phases(m, n, B)
    first, g0 = cells[0], geo[0]
    for x in range(len(cells)):
        for y in range(x + 1, len(cells)):
            (i1, j1), (i2, j2), a, b = cells[x], cells[y], geo[x], geo[y]
            if a["slot"] == b["slot"] and a["A"] != b["A"]:
                out.add("B1" if a["u"] == b["u"] else "B2")
            if a["A"] == b["A"] and a["slot"] != b["slot"]:
                out.add("B5")
            if i1 == i2:
                out.add("B6a")
            if j1 == j2:
                out.add("B6b")
    for (i, j), b in zip(cells[1:], geo[1:]):
        if b["lane"] == g0["lane"] and b["slot"] != g0["slot"] and i > first[0] and g0["A"] > b["A"]:
            out.add("B3")
        if b["lane"] != g0["lane"]:
            out.add("B4a" if g0["A"] > b["A"] else "B4b" if g0["A"] < b["A"] else "B5")
    if sum(a["A"] < head_end for a in geo) >= 2:
        out.add("B7h")
    if sum(a["A"] >= tail_start for a in geo) >= 2:
        out.add("B7t")
    if (m, n) in cells:
        out.add("B7l")
    if free is not None and free[0] != first and any(abs(i - j) > B - 1 and i < first[0] for i, j in free[1]):
        out.add("B8")
    if len(cells) >= 3 and len({a["lane"] for a in geo}) >= 3:
        out.add("B9")
    return out


def band_rules(cells, B, free_end):
    """the cell every wrong rule would report"""
    A = lambda c: c[0] + c[1]
    return {"earliest step, then smallest row": min(cells, key=lambda c: (A(c), c[0])),
            "column-major first": min(cells, key=lambda c: (c[1], c[0])),
            "last maximum": max(cells),
            "first maximum ignoring the band": free_end}


# ---------------------------------------------------------------------------------------------- b. the coupled LSW cases
RS = (2, 4, 8, 16)
FAMILIES = ("one stripe", "rolling")
LIN_CLASSES = ("L1", "L2", "L3", "L4", "L5", "L5adj", "L6col1", "L6coln", "L6row1", "L6rowm")
LIN_RULES = ("column-major first", "last maximum", "earliest wave step", "smallest column inside a lane before smallest row")
_ONE_STRIPE = "one stripe"
NO_SUCH_LIN_CASE = {(R, "one stripe"): {"L5": _ONE_STRIPE, "L5adj": _ONE_STRIPE} for R in RS}


def lin_shape(R, family):
    """one stripe with n < 128; three stripes (the last one partial) with n >= 128"""
    return (64 * R - 3, 120) if family == "one stripe" else (3 * 64 * R - 7, 150)


def lin_texts(R, family):
    m, n = lin_shape(R, family)
    s = 64 * R
    roll = family == "rolling"
    base = s if roll else 0                 # the classes of one stripe lie in stripe 1 of the rolling family
    lane = lambda l, r=0: base + l * R + r + 1   # row `r` of lane `l`
    dr = R - 1
    L = min(10, dr)                         # the longest motif that fits between the first and the last row of a lane
    far = lane(63) if roll else lane(61)    # (the last lane of the single stripe holds R - 3 rows)
    cases = [
        ("lower row of a lane at the smaller column", pair(m, n, [(0, L, lane(20), 60), (1, L, lane(20, dr), 40)])),
        ("upper row of a lane at the smaller column", pair(m, n, [(0, L, lane(20), 40), (1, L, lane(20, dr), 95)])),
        ("one row, two columns", pair(m, n, [(0, 10, lane(9, 1), 40)], ref=[(0, 10, 70)])),
        ("later lane at the smaller column", pair(m, n, [(0, 10, lane(9, 1), 80), (1, 10, lane(9, 1) + 16, 40)])),
        ("rows of lane 0", pair(m, n, [(0, 1, 1 + (2 * s if roll else 0), 77), (1, 1, R + (2 * s if roll else 0), 23)])),
        ("row 1 and column 1", pair(m, n, [(0, 1, 1, 50), (1, 1, 30, 1)])),
        ("far lanes, the later at the smaller column", pair(m, n, [(0, 10, lane(5), 100), (1, 10, far, 12)])),
        ("column n and row m", pair(m, n, [(0, 10, 60, n), (1, 10, m, 70)])),
        ("control: unique maximum", pair(m, n, [(0, 10, lane(9), 30), (1, 5, lane(9) + 30, 50)])),
        ("control: score 0", pair(m, n)),
        ("control: unique maximum at (m, n)", pair(m, n, [(0, 10, m, n)])),
        ("one row, three columns", pair(m, n, [(0, 10, lane(33, dr), 25)], ref=[(0, 10, 61), (0, 10, 110)])),
    ]
    if roll:
        cases += [
            ("last row of stripe 0, first of stripe 1", pair(m, n, [(0, 1, s, 80), (1, 1, s + 1, 40)])),
            ("stripe 0 and stripe 2, the later at the smaller column", pair(m, n, [(0, 10, 50, 90), (1, 10, 2 * s + 20, 30)])),
        ]
        for k, (ref, qry) in enumerate(tie_texts(R)):   # score_only_cases' ties across stripes, padded to the family's shape
            assert len(qry) <= m and len(ref) <= n
            cases.append(("score_only_cases.tie_texts[%d]" % k, (ref + b"y" * (n - len(ref)), qry + b"x" * (m - len(qry)))))
    assert len(cases) % 2 == 0 and 12 <= len(cases) <= 24 and all(len(r) == n and len(q) == m for _, (r, q) in cases)
    return cases


def lin_classes(cells, R, m, n):
    out = set()
    if len(cells) < 2:
        return out
    geo = [stripe_geo(i, j, n, R) for i, j in cells]
    (i0, j0), g0 = cells[0], geo[0]
    for (i, j), b in zip(cells[1:], geo[1:]):
        same_lane = (b["stripe"], b["lane"]) == (g0["stripe"], g0["lane"])
        if same_lane and i > i0:
            out.add("L1" if j < j0 else "L2" if j > j0 else "col")
        if i == i0:
            out.add("L3")
        if b["stripe"] == g0["stripe"] and b["lane"] > g0["lane"] and j < j0:
            out.add("L4")
        if b["stripe"] > g0["stripe"] and j < j0:
            out.add("L5")
            if i == i0 + 1:
                out.add("L5adj")
    for i, j in cells:
        out |= {"L6col1"} if j == 1 else set()
        out |= {"L6coln"} if j == n else set()
        out |= {"L6row1"} if i == 1 else set()
        out |= {"L6rowm"} if i == m else set()
    return out - {"col"}


def lin_rules(cells, R, n):
    geo = {c: stripe_geo(c[0], c[1], n, R) for c in cells}
    return {"column-major first": min(cells, key=lambda c: (c[1], c[0])),
            "last maximum": max(cells),
            "earliest wave step": min(cells, key=lambda c: (geo[c]["T"], c[0])),
            "smallest column inside a lane before smallest row": min(cells, key=lambda c: (geo[c]["stripe"], geo[c]["lane"], c[1], c[0]))}


# ---------------------------------------------------------------------------------------------- expectations
def want(ref, qry, band=0):
    """what the GPU must report for one pair, from oracle_py.lsw alone; `cells` (the tied cells) labels failure messages"""
    o = O.lsw(ref, qry, *W, band=band)
    _, cells = tied_cells(o.H, band)
    lines = ("", "", "") if o.score == 0 else O.lsw_traceback(ref, qry, o)
    return {"score": o.score, "end": (o.end_row, o.end_col), "lines": lines, "cells": cells, "H": o.H}


def band_case(B):
    """(names, texts, expectations, per-pair classes) of one band"""
    def build():
        m, n = band_shape(B)
        names, texts = zip(*band_texts(B))
        exp = [want(r, q, B) for r, q in texts]
        cls = []
        for (r, q), e in zip(texts, exp):
            f = O.lsw(r, q, *W, want_dir=False)
            e["free_end"] = (f.end_row, f.end_col)
            cls.append(sorted(band_classes(e["cells"], B, m, n, (e["free_end"], tied_cells(f.H)[1]))))
        for p, e in enumerate(exp):
            if p not in MATRIX_PAIRS:
                del e["H"]
        return list(names), list(texts), exp, cls
    return shared(("tie band", B), build)


def lin_case(R, family):
    def build():
        m, n = lin_shape(R, family)
        names, texts = zip(*lin_texts(R, family))
        exp = [want(r, q) for r, q in texts]
        for e in exp:
            del e["H"]   # (no linear test compares whole matrices)
        cls = [sorted(lin_classes(e["cells"], R, m, n)) for e in exp]
        return list(names), list(texts), exp, cls
    return shared(("tie lsw", R, family), build)
