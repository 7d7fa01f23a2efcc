"""tests/lb2_oracle.c, the oracle of two-piece local band-direction batches (BASW), checked two ways on the CPU:
1. with equal pieces it reports, cell for cell, what the one-piece oracles report (tests/bdl_oracle.c and tests/bdlt_oracle.c through
   their _ref modules): score, end cell, lines and the H / I / D planes, over their fuzz sets, with and without a table; piece 2's planes
   equal piece 1's;
2. with unequal pieces its H equals a numpy DP that enumerates gap lengths under the local rules -- zero floor; a gap run may start from
   an in-band cell's H or from the first cell without a code above / left of the run, which reads 0; the diagonal from a border cell reads
   0 -- on pairs up to 60 x 60 at bands 1..40; its lines rescore to its score, and two pieces beat one in several cases."""
import numpy as np
import pytest

import bdl_ref
import bdlt_ref
import lb2_ref
import zsub_ref
from bdl_ref import BASW
from test_bd2_oracle import PIECES
from test_bdl_oracle import BANDS, WEIGHTS, _pairs
from test_bdlt_oracle import _byte_pairs


@pytest.fixture(scope="module")
def orc(tmp_path_factory):
    return lb2_ref.build(tmp_path_factory.mktemp("lb2_oracle"))


@pytest.fixture(scope="module")
def bdl(tmp_path_factory):
    return bdl_ref.build(tmp_path_factory.mktemp("lb2_oracle_bdl"))


@pytest.fixture(scope="module")
def bdlt(tmp_path_factory):
    return bdlt_ref.build(tmp_path_factory.mktemp("lb2_oracle_bdlt"))


def _same_as_one_piece(got, want, tag):
    assert (got["score"], got["end"], got["lines"]) == (want["score"], want["end"], want["lines"]), tag
    for key, have in zip(("dirH", "dirI", "dirD"), got["dirs"][:3]):
        assert np.array_equal(have, want[key]), (tag, key)
    assert np.array_equal(got["dirs"][3], got["dirs"][1]) and np.array_equal(got["dirs"][4], got["dirs"][2]), tag
    # a piece is named exactly where H's move is a gap
    assert np.array_equal(got["dirs"][5] > 0, got["dirs"][0] >= 3), tag


@pytest.mark.parametrize("alphabet", [2, 256])
def test_equal_pieces_are_the_one_piece_definition(orc, bdl, alphabet):
    cases = 0
    for wi, w in enumerate(WEIGHTS):
        for ref, qry in _pairs(alphabet, 40, 100 * alphabet + wi):  # (tests/test_bdl_oracle.py's set)
            for band in BANDS:
                want = bdl.align(BASW, ref, qry, w, band, planes=True)
                got = orc.align(ref, qry, w[:2], w[2:], w[2:], band, planes=True)
                _same_as_one_piece(got, want, (w, band, ref, qry))
                cases += 1
    assert cases >= 100


def test_equal_pieces_under_a_table_are_the_one_piece_definition(orc, bdlt):
    cases = 0
    for seed in (1, 2):  # (tests/test_bdlt_oracle.py's set: asymmetric 32-code tables holding -128 and 127, bytes of the whole range)
        table = bdlt_ref.random_table(seed)
        g = ((-3, -1), (-7, -2))[seed - 1]
        for ref, qry in _byte_pairs(16, 40 * BASW + seed):
            for band in (1, 2, 5, 16, 33):
                want = bdlt.align(BASW, ref, qry, table, g, band, planes=True)
                got = orc.align(ref, qry, table, g, g, band, planes=True)
                _same_as_one_piece(got, want, (seed, band, ref, qry))
                cases += 1
    table = bdlt_ref.dna_table()
    for ref, qry in _pairs(4, 20, 77):
        for band in BANDS:
            want = bdlt.align(BASW, ref, qry, table, (-5, -1), band, planes=True)
            got = orc.align(ref, qry, table, (-5, -1), (-5, -1), band, planes=True)
            _same_as_one_piece(got, want, ("dna", band, ref, qry))
            cases += 1
    assert cases >= 100


def _enumerating_dp(ref, qry, scores, code, p1, p2, B):
    """H over the band by enumerating gap lengths under the local rules; 0 on the borders and outside the band"""
    m, n = len(qry), len(ref)
    H = np.zeros((m + 1, n + 1), np.int64)
    g = np.array([0] + [lb2_ref.gap(k, p1, p2) for k in range(1, max(m, n) + 1)], np.int64)
    has_code = lambda i, j: i >= 1 and j >= 1 and abs(i - j) <= B - 1
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            if not has_code(i, j):
                continue
            best = max(0, H[i - 1, j - 1] + int(scores[code[ref[j - 1]]][code[qry[i - 1]]]))  # (a border or out-of-band corner holds 0)
            for k in range(1, i + 1):  # a run of k deletions: through cells with a code, from the first source without one at the latest
                if has_code(i - k, j):
                    best = max(best, H[i - k, j] + g[k])
                else:
                    best = max(best, g[k])
                    break
            for k in range(1, j + 1):
                if has_code(i, j - k):
                    best = max(best, H[i, j - k] + g[k])
                else:
                    best = max(best, g[k])
                    break
            H[i, j] = best
    return H


def test_h_equals_the_gap_length_enumeration(orc):
    rng = np.random.default_rng(2027)
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
            got = orc.align(ref, qry, (table, code), p1, p2, band, planes=True, h=True)
            want = _enumerating_dp(ref, qry, table, code, p1, p2, band)
            assert np.array_equal(got["H"], want), (band, p1, p2, ref, qry, np.argwhere(got["H"] != want)[:4])
            # the score is the first maximum of H in row-major order, (0, 0) when every H is 0
            top = int(want.max())
            assert got["score"] == top, (band, p1, p2)
            assert got["end"] == (tuple(int(x) for x in np.argwhere(want == top)[0]) if top > 0 else (0, 0)), (band, p1, p2)
            assert np.array_equal(got["dirs"][0] == 0, want == 0), (band, p1, p2)  # NONE exactly where H == 0
            if max(p1[0], p1[1], p2[0], p2[1]) <= 0:  # (with a positive weight, merging two adjacent gaps of one kind may score differently)
                assert lb2_ref.rescore(got["lines"], (table, code), p1, p2)[0] == got["score"], (band, p1, p2, got["lines"])
            one = orc.align(ref, qry, (table, code), p1, p1, band)
            assert got["score"] >= one["score"]  # (a second piece only adds paths)
            two_wins += got["score"] > one["score"]
            cases += 1
    assert cases >= 80 and two_wins >= 5, (cases, two_wins)
