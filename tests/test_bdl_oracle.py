"""The band-only oracle tests/bdl_oracle.c (BSW and BASW in O((m + n) * B) memory, what the long-pair GPU tests are checked against)
against the full-matrix oracles it must agree with: tests/basw_oracle.c for BASW, and orc_bsw_fill with the LSW walk (oracle/, through
tests/oracle_py.py) for BSW.  Scores, end cells, the three lines and every exported enum plane, cell for cell.  CPU only."""
import numpy as np
import pytest

import basw_ref
import bdl_ref
import oracle_py
from bdl_ref import BASW, BSW

WEIGHTS = [(3, -1, -2, -1), (1, -1, -1, -1), (2, -3, 0, -1), (0, 0, 0, 0), (5, 2, -4, -2), (1, -2, 1, -3), (7, -5, -9, 1)]  # tests/test_gpu_fuzz.py's
BANDS = [1, 2, 3, 7, 16, 200]  # (200 covers every pair here)


@pytest.fixture(scope="module")
def bdl(tmp_path_factory):
    return bdl_ref.build(tmp_path_factory.mktemp("bdl_oracle"))


@pytest.fixture(scope="module")
def basw(tmp_path_factory):
    return basw_ref.build(tmp_path_factory.mktemp("bdl_oracle_basw"))


def _pairs(alphabet, count, seed):
    """random pairs of 0-90 bases, half of them related (a mutated copy with indels), and the edge cases: empty strings, single bases,
    one repeated base (every maximum tied), and a pair with no base in common (every H is 0 under negative mismatches)"""
    rng = np.random.default_rng(seed)
    base = 65 if alphabet <= 26 else 0
    out = [(b"", b""), (b"", b"ACGT"), (b"ACGT", b""), (b"A", b"A"), (b"A", b"C"), (b"A" * 40, b"A" * 33), (b"A" * 30, b"C" * 30)]
    for k in range(count):
        n, m = int(rng.integers(0, 91)), int(rng.integers(0, 91))
        ref = (rng.integers(0, alphabet, n) + base).astype(np.uint8)
        if k % 2 and n:
            q = ref.copy()
            sub = rng.random(n) < 0.1
            q[sub] = (rng.integers(0, alphabet, int(sub.sum())) + base).astype(np.uint8)
            q = q[~(rng.random(n) < 0.05)]
            cut = int(rng.integers(0, len(q) + 1))
            q = np.concatenate([q[:cut], (rng.integers(0, alphabet, int(rng.integers(0, 6))) + base).astype(np.uint8), q[cut:]])[:90]
        else:
            q = (rng.integers(0, alphabet, m) + base).astype(np.uint8)
        out.append((ref.tobytes(), q.astype(np.uint8).tobytes()))
    return out


@pytest.mark.parametrize("alphabet", [2, 256])
def test_basw_agrees_with_the_full_matrix_oracle(bdl, basw, alphabet):
    n_checked = 0
    for wi, w in enumerate(WEIGHTS):
        for ref, qry in _pairs(alphabet, 40, 100 * alphabet + wi):
            for band in BANDS:
                want = basw.align(ref, qry, *w, band)
                got = bdl.align(BASW, ref, qry, w, band, planes=True)
                assert (got["score"], got["end"], got["lines"]) == (want["score"], want["end"], want["lines"]), (w, band, ref, qry)
                for key in ("dirH", "dirI", "dirD"):
                    assert np.array_equal(got[key], want[key]), (w, band, key, ref, qry)
                n_checked += 1
    assert n_checked >= 7 * 47 * 6


@pytest.mark.parametrize("alphabet", [2, 256])
def test_bsw_agrees_with_the_full_matrix_oracle(bdl, alphabet):
    zero_t = 0
    for wi, w in enumerate(WEIGHTS):
        for ref, qry in _pairs(alphabet, 40, 100 * alphabet + 50 + wi):
            for band in BANDS:
                want = oracle_py.lsw(ref, qry, *w[:3], band=band)
                got = bdl.align(BSW, ref, qry, w, band, planes=True)
                assert (got["score"], got["end"]) == (want.score, (want.end_row, want.end_col)), (w, band, ref, qry)
                assert np.array_equal(got["dirH"], want.dir), (w, band, ref, qry)
                assert not got["dirI"].any() and not got["dirD"].any()
                assert tuple(x.decode("latin-1") for x in got["lines"]) == oracle_py.lsw_traceback(ref, qry, want), (w, band, ref, qry)
                zero_t += int(((want.H == 0) & (want.dir != 0)).sum())
    assert zero_t > 0  # cells with t == 0: H is 0 and the move is not NONE


def test_a_long_pair_is_cheap_and_consistent(bdl):
    """33 000 bases at band 64 (a full matrix would be 10^9 cells): the end cell lies in the band, the lines spell substrings of the two
    strings that end at it, and the score is the lines' own score"""
    rng = np.random.default_rng(5)
    ref = (rng.integers(0, 4, 33000) + 65).astype(np.uint8)
    q = ref.copy()
    sub = rng.random(33000) < 0.05
    q[sub] = (rng.integers(0, 4, int(sub.sum())) + 65).astype(np.uint8)
    ref, qry = ref.tobytes(), q.tobytes()
    for algo, w in ((BSW, (3, -1, -2)), (BASW, (3, -1, -3, -1))):
        r = bdl.align(algo, ref, qry, w, 64)
        (i, j), (lr, lx, lq) = r["end"], r["lines"]
        assert r["score"] > 32767 and abs(i - j) <= 63
        rs, qs = lr.replace(b"_", b""), lq.replace(b"_", b"")
        assert ref[j - len(rs):j] == rs and qry[i - len(qs):i] == qs
        score, gap = 0, None
        for a, x, b in zip(lr, lx, lq):
            if x == ord("*") or x == ord("|"):
                score, gap = score + (w[0] if a == b else w[1]), None
            else:
                side = "i" if b == ord("_") else "d"
                score += w[2] if algo == BSW else (w[3] if gap == side else w[2] + w[3])
                gap = side
        assert score == r["score"]
