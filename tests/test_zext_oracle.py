"""The CPU oracle of BAXT's extension mode (tests/zext_oracle.c) against BAXT's oracle where the mode is off or cannot act, against the
properties the definition implies, and against a brute-force Python restatement of include/dpx_align.h on the fuzz set; and the fuzz
set itself: every class of pair the GPU tests rely on is present in it."""
import numpy as np
import pytest

import baxt_ref
import zext_ref
from zext_ref import FUZZ_E, FUZZ_WEIGHTS, FUZZ_Z, NO_QUERY_END, REACHED_END, ZDROPPED

NEG = None  # -infinity of the restatement


@pytest.fixture(scope="module")
def zext(tmp_path_factory):
    return zext_ref.build(tmp_path_factory.mktemp("zext_oracle"))


@pytest.fixture(scope="module")
def baxt(tmp_path_factory):
    return baxt_ref.build(tmp_path_factory.mktemp("zext_baxt_oracle"))


@pytest.fixture(scope="module")
def fuzz():
    return zext_ref.fuzz_texts()


def _pairs(fuzz):
    return [(band, ref, qry) for band, texts in fuzz.items() for ref, qry in texts]


def brute(ref, qry, w, B, Z, E):
    """the header's definition, cell by cell: (record fields as a dict, chosen score, chosen end, (bi, bj))"""
    ma, mi, o, e = w
    m, n = len(qry), len(ref)
    inb = lambda i, j: abs(i - j) <= B - 1
    add = lambda x, y: NEG if x is NEG else x + y
    big = lambda x, y: y if x is NEG else x if y is NEG else max(x, y)
    H, I, D = ({} for _ in range(3))
    for i in range(m + 1):
        for j in range(n + 1):
            if not inb(i, j):
                continue
            if i == 0 or j == 0:
                H[i, j] = 0 if i == j else o + (i + j) * e
                continue
            D[i, j] = big(add(H.get((i - 1, j), NEG), o + e), add(D.get((i - 1, j), NEG), e))
            I[i, j] = big(add(H.get((i, j - 1), NEG), o + e), add(I.get((i, j - 1), NEG), e))
            H[i, j] = big(big(D[i, j], I[i, j]), H[i - 1, j - 1] + (ma if qry[i - 1] == ref[j - 1] else mi))
    pen = -e if e < 0 else 0
    best, bi, bj, last, dropped = 0, 0, 0, m + n, False
    for a in range(1, m + n + 1):
        cells = [(i, a - i) for i in range(m + 1) if 0 <= a - i <= n and inb(i, a - i)]
        if not cells:
            continue
        dm = max(H[c] for c in cells)
        ia, ja = next(c for c in cells if H[c] == dm)
        if dm > best:
            best, bi, bj = dm, ia, ja
        elif Z >= 0 and ia >= bi and ja >= bj and best - dm > Z + pen * abs((ia - bi) - (ja - bj)):
            last, dropped = a, True
            break
    done = sorted(c for c in H if c[0] + c[1] <= last)  # row-major
    mx = max(max(H[c] for c in done), 0)
    mcell = next(c for c in done if H[c] == mx) if mx > 0 else (0, 0)
    row = [c for c in done if c[0] == m]
    qe = max(H[c] for c in row) if row else NO_QUERY_END
    qj = next(c[1] for c in row if H[c] == qe) if row else -1
    reached = E >= 0 and not dropped and bool(row) and qe + E > mx
    rec = dict(maxScore=mx, maxRow=mcell[0], maxCol=mcell[1], qryEndScore=qe, qryEndCol=qj, lastDiag=last,
               flags=(ZDROPPED if dropped else 0) | (REACHED_END if reached else 0), reserved=0)
    return rec, (qe if reached else mx), ((m, qj) if reached else mcell), (bi, bj)


@pytest.mark.parametrize("w", FUZZ_WEIGHTS)
def test_off_and_huge_z_are_baxt(zext, baxt, fuzz, w):
    for band, ref, qry in _pairs(fuzz):
        want = baxt.align(ref, qry, *w, band, raw=False)
        for Z in (-1, 1 << 30):
            got = zext.align(ref, qry, *w, band, Z, -1)
            assert (got["score"], got["end"], got["lines"]) == (want["score"], want["end"], want["lines"]), (w, band, ref, qry, Z)
            assert got["rec"]["lastDiag"] == len(ref) + len(qry) and got["rec"]["flags"] == 0
            assert (got["rec"]["maxScore"], got["rec"]["maxRow"], got["rec"]["maxCol"]) == (want["score"],) + want["end"]
            for key in ("H", "I", "D"):
                assert np.array_equal(got[key], want[key]), (w, band, key)


@pytest.mark.parametrize("w", FUZZ_WEIGHTS)
def test_monotone_in_z_and_never_above_baxt(zext, baxt, fuzz, w):
    for band, ref, qry in _pairs(fuzz):
        full = baxt.result(ref, qry, w, band)[0]
        lasts = []
        for Z in (0, 1, 2, 4, 6, 10, 1 << 30):
            r = zext.align(ref, qry, *w, band, Z, -1, walk=False)["rec"]
            assert r["maxScore"] <= full, (w, band, ref, qry, Z)
            lasts.append(r["lastDiag"])
        assert lasts == sorted(lasts), (w, band, ref, qry, lasts)


@pytest.mark.parametrize("w", FUZZ_WEIGHTS)
def test_agrees_with_the_restatement(zext, fuzz, w):
    for band, ref, qry in _pairs(fuzz):
        for Z, E in [(z, FUZZ_E) for z in FUZZ_Z] + [(-1, 0), (2, -1)]:
            got = zext.align(ref, qry, *w, band, Z, E, walk=False)
            rec, score, end, bcell = brute(ref, qry, w, band, Z, E)
            assert (got["rec"], got["score"], got["end"], got["best_cell"]) == (rec, score, end, bcell), (w, band, ref, qry, Z, E)


@pytest.mark.parametrize("w", FUZZ_WEIGHTS)
def test_the_fuzz_set_holds_every_class(zext, fuzz, w):
    """what the GPU fuzz test relies on.  A drop at lastDiag = 1 needs best - (o + e) > Z + pen at best = 0, Z = 0: only weights with
    -(o + e) > pen can produce it.  (bi, bj) != (maxRow, maxCol) was found under (2, -1, 1, -1) only; the seed keeps one."""
    at1 = past1 = reached = norow = differ = 0
    for band, ref, qry in _pairs(fuzz):
        for Z in FUZZ_Z:
            got = zext.align(ref, qry, *w, band, Z, FUZZ_E, walk=False)
            r = got["rec"]
            at1 += bool(r["flags"] & ZDROPPED) and r["lastDiag"] == 1
            past1 += bool(r["flags"] & ZDROPPED) and r["lastDiag"] > 1
            reached += bool(r["flags"] & REACHED_END)
            norow += r["qryEndCol"] < 0 and r["qryEndScore"] == NO_QUERY_END
            differ += got["best_cell"] != (r["maxRow"], r["maxCol"]) and r["maxScore"] > 0
    print(w, dict(at1=at1, past1=past1, reached=reached, norow=norow, differ=differ))
    o, e = w[2], w[3]
    if -(o + e) > (-e if e < 0 else 0):
        assert at1 >= 1, w
    assert past1 >= 1 and reached >= 1 and norow >= 1, (w, past1, reached, norow)
    if w == (2, -1, 1, -1):
        assert differ >= 1, differ
