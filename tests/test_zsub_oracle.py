"""The CPU oracle of BAXT's extension mode under a substitution table (tests/zsub_oracle.c) against the two oracles whose conjunction
it is -- zext_oracle.c under an identity table, subst_oracle.c (BAXT's end) with the mode off -- and against a brute-force Python
restatement of include/dpx_align.h on the fuzz set; and the fuzz set itself: every class of pair the GPU tests rely on is in it."""
import numpy as np
import pytest

import subst_ref
import zext_ref
import zsub_ref
from zsub_ref import FUZZ_E, FUZZ_GAPS, FUZZ_TABLES, FUZZ_Z, NO_QUERY_END, REACHED_END, ZDROPPED

NEG = None  # -infinity of the restatement


@pytest.fixture(scope="module")
def zsub(tmp_path_factory):
    return zsub_ref.build(tmp_path_factory.mktemp("zsub_oracle"))


@pytest.fixture(scope="module")
def zext(tmp_path_factory):
    return zext_ref.build(tmp_path_factory.mktemp("zsub_zext_oracle"))


@pytest.fixture(scope="module")
def subst(tmp_path_factory):
    return subst_ref.build(tmp_path_factory.mktemp("zsub_subst_oracle"))


@pytest.fixture(scope="module")
def fuzz():
    return zsub_ref.fuzz_texts()


def _pairs(fuzz):
    return [(band, ref, qry) for band, texts in fuzz.items() for ref, qry in texts]


def brute(ref, qry, table, code, gaps, B, Z, E):
    """the header's definition, cell by cell: (record fields as a dict, chosen score, chosen end, (bi, bj))"""
    o, e = gaps
    m, n = len(qry), len(ref)
    inb = lambda i, j: abs(i - j) <= B - 1
    add = lambda x, y: NEG if x is NEG else x + y
    big = lambda x, y: y if x is NEG else x if y is NEG else max(x, y)
    s = lambda r, q: int(table[int(code[r])][int(code[q])])  # the row is the reference code
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
            H[i, j] = big(big(D[i, j], I[i, j]), H[i - 1, j - 1] + s(ref[j - 1], qry[i - 1]))
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


@pytest.mark.parametrize("w", zext_ref.FUZZ_WEIGHTS)
def test_identity_table_is_zext(zsub, zext, w):
    """bit for bit: records, chosen score and end, the scan's cell, all three planes and the lines, on zext's fuzz set"""
    for band, ref, qry in _pairs(zext_ref.fuzz_texts()):
        table, code = subst_ref.identity_table(w[0], w[1], ref + qry)
        for Z in zext_ref.FUZZ_Z:
            for E in (zext_ref.FUZZ_E, -1):
                want = zext.align(ref, qry, *w, band, Z, E)
                got = zsub.align(ref, qry, table, code, w[2], w[3], band, Z, E)
                assert sorted(got) == sorted(want)
                for key in ("rec", "score", "end", "best_cell", "lines"):
                    assert got[key] == want[key], (w, band, ref, qry, Z, E, key)
                for key in ("H", "I", "D"):
                    assert np.array_equal(got[key], want[key]), (w, band, ref, qry, Z, E, key)
        want = zext.align(ref, qry, *w, band, -1, zext_ref.FUZZ_E)
        got = zsub.align(ref, qry, table, code, w[2], w[3], band, -1, zext_ref.FUZZ_E)
        assert all(got[k] == want[k] for k in ("rec", "score", "end", "best_cell", "lines")), (w, band, ref, qry)


@pytest.mark.parametrize("table", FUZZ_TABLES)
def test_mode_off_is_subst_with_baxt_end(zsub, subst, table):
    """Z = E = -1, which the oracle accepts and the ABI does not: subst_oracle.c with ext = True, on its fuzz pairs"""
    code = subst_ref.fuzz_code()
    for band in range(1, 6):
        for ref, qry in subst_ref.fuzz_pairs(band, banw=False):
            want = subst.align(ref, qry, table, code, *FUZZ_GAPS, band, ext=True)
            got = zsub.align(ref, qry, table, code, *FUZZ_GAPS, band, -1, -1)
            assert (got["score"], got["end"], got["lines"]) == (want["score"], want["end"], want["lines"]), (table, band, ref, qry)
            assert got["rec"]["lastDiag"] == len(ref) + len(qry) and got["rec"]["flags"] == 0
            assert (got["rec"]["maxScore"], got["rec"]["maxRow"], got["rec"]["maxCol"]) == (want["score"],) + want["end"]
            for key in ("H", "I", "D"):
                assert np.array_equal(got[key], want[key]), (table, band, ref, qry, key)


@pytest.mark.parametrize("table", FUZZ_TABLES)
def test_agrees_with_the_restatement(zsub, fuzz, table):
    code = subst_ref.fuzz_code()
    for band, ref, qry in _pairs(fuzz):
        for Z in FUZZ_Z:
            got = zsub.align(ref, qry, table, code, *FUZZ_GAPS, band, Z, FUZZ_E, walk=False)
            rec, score, end, bcell = brute(ref, qry, table, code, FUZZ_GAPS, band, Z, FUZZ_E)
            assert (got["rec"], got["score"], got["end"], got["best_cell"]) == (rec, score, end, bcell), (table, band, ref, qry, Z)


def test_the_fuzz_set_holds_every_class(zsub, fuzz):
    """what the GPU fuzz test relies on, over the whole set (all tables, all Z): a dropped pair, a reached-end pair, a pair with
    DPX_EXT_NO_QUERY_END, a pair whose scan cell differs from (maxRow, maxCol), and a pair whose record changes when the asymmetric
    table is transposed"""
    code = subst_ref.fuzz_code()
    dropped = reached = norow = differ = transposed = 0
    for table in FUZZ_TABLES:
        flipped = np.asarray(table).T
        for band, ref, qry in _pairs(fuzz):
            for Z in FUZZ_Z:
                got = zsub.align(ref, qry, table, code, *FUZZ_GAPS, band, Z, FUZZ_E, walk=False)
                r = got["rec"]
                dropped += bool(r["flags"] & ZDROPPED)
                reached += bool(r["flags"] & REACHED_END)
                norow += r["qryEndCol"] < 0 and r["qryEndScore"] == NO_QUERY_END
                differ += got["best_cell"] != (r["maxRow"], r["maxCol"]) and r["maxScore"] > 0
                if not np.array_equal(flipped, table):
                    transposed += zsub.align(ref, qry, flipped, code, *FUZZ_GAPS, band, Z, FUZZ_E, walk=False)["rec"] != r
    print(dict(dropped=dropped, reached=reached, norow=norow, differ=differ, transposed=transposed))
    assert dropped >= 1 and reached >= 1 and norow >= 1 and differ >= 1 and transposed >= 1, (dropped, reached, norow, differ, transposed)
