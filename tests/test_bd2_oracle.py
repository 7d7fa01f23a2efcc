"""tests/bd2_oracle.c, the oracle of two-piece band-direction batches, checked two ways on the CPU:
1. with equal pieces it reports, cell for cell, what the one-piece oracles report (tests/zsub_oracle.c through bdx_ref.expect): record,
   chosen score and end cell, lines and the H / I / D planes, over the fuzz set in all eight modes; piece 2's planes equal piece 1's;
2. with unequal pieces its H equals a numpy DP that enumerates gap lengths, H = max(diag, max_k H[i-k][j] + g(k), max_k H[i][j-k] + g(k))
   over in-band cells, on pairs up to 60 x 60 at bands 1..40; and its lines rescore to its score."""
import numpy as np
import pytest

import bd2_ref
import bdx_ref
import subst_ref
import zsub_ref
from bd2_ref import BANW, BAXT, MODES


@pytest.fixture(scope="module")
def orc(tmp_path_factory):
    return bd2_ref.build(tmp_path_factory.mktemp("bd2_oracle"))


@pytest.fixture(scope="module")
def zs(tmp_path_factory):
    return zsub_ref.build(tmp_path_factory.mktemp("bd2_oracle_zs"))


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_equal_pieces_are_the_one_piece_definition(orc, zs, mode):
    _, algo, with_table, drop, bonus = mode
    code = subst_ref.fuzz_code()
    gaps = zsub_ref.FUZZ_GAPS
    cases = 0
    for band, texts in zsub_ref.fuzz_texts().items():
        for table in zsub_ref.FUZZ_TABLES:
            if not with_table and table[0][1] != table[1][0]:
                continue  # (not a match / mismatch pair)
            tab = np.array(table, np.int8)
            for z in (zsub_ref.FUZZ_Z if drop else (-1,)):
                e = zsub_ref.FUZZ_E if bonus else -1
                for ref, qry in texts:
                    if algo == BANW and abs(len(ref) - len(qry)) >= band:
                        continue
                    want = bdx_ref.expect(zs, ref, qry, tab, code, *gaps, band, algo == BAXT, z, e)
                    got = orc.expect(ref, qry, tab, code, gaps, gaps, band, algo == BAXT, z, e)
                    tag = (mode[0], band, table, z, ref, qry)
                    assert (got["rec"], got["score"], got["end"], got["lines"]) == (want["rec"], want["score"], want["end"], want["lines"]), tag
                    for key, have, exp in zip("HID", got["dirs"][:3], want["dirs"]):
                        assert np.array_equal(have, exp), (tag, key)
                    assert np.array_equal(got["dirs"][3], got["dirs"][1]) and np.array_equal(got["dirs"][4], got["dirs"][2]), tag
                    gapped = (got["dirs"][0] >= 3) & (got["dirs"][5] > 0)  # (border cells of H carry a gap enum and no piece)
                    assert np.array_equal(got["dirs"][5] > 0, gapped), tag
                    cases += 1
    assert cases >= 100


def _enumerating_dp(ref, qry, scores, code, p1, p2, B):
    """H over the band by enumerating gap lengths; NEG_INF outside the band"""
    m, n = len(qry), len(ref)
    neg = bd2_ref.NEG_INF
    H = np.full((m + 1, n + 1), neg, np.int64)
    g = np.array([0] + [bd2_ref.gap(k, p1, p2) for k in range(1, max(m, n) + 1)], np.int64)
    for i in range(m + 1):
        for j in range(n + 1):
            if abs(i - j) > B - 1:
                continue
            if i == 0 or j == 0:
                H[i, j] = g[i + j]
                continue
            best = H[i - 1, j - 1] + int(scores[code[ref[j - 1]]][code[qry[i - 1]]])
            for k in range(1, i + 1):
                if abs(i - k - j) <= B - 1:
                    best = max(best, H[i - k, j] + g[k])
            for k in range(1, j + 1):
                if abs(i - j + k) <= B - 1:
                    best = max(best, H[i, j - k] + g[k])
            H[i, j] = best
    return H


PIECES = [((-4, -2), (-24, -1)), ((-2, -3), (-9, -1)), ((-24, -1), (-4, -2)), ((0, -2), (-5, 0)), ((-3, -1), (-3, -1)), ((1, -3), (-4, 1))]


def test_h_equals_the_gap_length_enumeration(orc):
    rng = np.random.default_rng(2026)
    table, code = zsub_ref.acgtn_table()
    acgt = np.frombuffer(b"ACGT", np.uint8)
    cases, two_wins = 0, 0
    for band in list(range(1, 41, 3)) + [2, 40]:
        for p1, p2 in PIECES:
            n, m = int(rng.integers(0, 61)), int(rng.integers(0, 61))
            ref = acgt[rng.integers(0, 4, n)]
            qry = np.resize(ref, m).copy() if n else acgt[rng.integers(0, 4, m)]
            if m > 20:  # a deletion long enough for piece 2, and noise
                qry = np.concatenate([qry[:m // 3], qry[m // 3 + min(band - 1, 12):], acgt[rng.integers(0, 4, 12)]])[:m]
            ref, qry = ref.tobytes(), qry.tobytes()
            got = orc.expect(ref, qry, table, code, p1, p2, band, True, h=True)
            want = _enumerating_dp(ref, qry, table, code, p1, p2, band)
            assert np.array_equal(got["H"], want), (band, p1, p2, ref, qry, np.argwhere(got["H"] != want)[:4])
            # the score is the first maximum of H above 0 in row-major order, and the lines rescore to it between (0, 0) and the end cell
            top = int(want.max())
            assert got["score"] == max(top, 0), (band, p1, p2)
            if top > 0:
                assert got["end"] == tuple(int(x) for x in np.argwhere(want == top)[0]), (band, p1, p2)
            if max(p1[0], p1[1], p2[0], p2[1]) <= 0:  # (with a positive weight, merging two adjacent gaps of one kind may score differently)
                assert bd2_ref.rescore(got["lines"], table, code, p1, p2) == (got["score"], *got["end"]), (band, p1, p2, got["lines"])
            if abs(m - n) < band:
                gw = orc.expect(ref, qry, table, code, p1, p2, band, False)
                assert gw["score"] == int(want[m, n]) and gw["end"] == (m, n)
                one = orc.expect(ref, qry, table, code, p1, p1, band, False)
                two_wins += gw["score"] > one["score"]
            cases += 1
    assert cases >= 80 and two_wins >= 5
