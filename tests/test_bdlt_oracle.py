"""The band-only table oracle tests/bdlt_oracle.c (BSW and BASW under a substitution table in O((m + n) * B) memory, what the k_bdlt_fill
GPU tests are checked against) against three things it must agree with: tests/bdl_oracle.c under a table equivalent to match / mismatch,
tests/dirtab_oracle.c's ASW at a covering band, and a plain full-matrix recurrence written here from the definition in
include/dpx_align.h.  Scores, end cells, the three lines and every exported enum plane, cell for cell.  CPU only."""
import numpy as np
import pytest

import bdl_ref
import bdlt_ref
import dirtab_ref
from bdlt_ref import BASW, BSW
from test_bdl_oracle import BANDS, WEIGHTS, _pairs

LETTERS = bytes(range(65, 91))  # the letters _pairs draws from at alphabets <= 26


@pytest.fixture(scope="module")
def bdlt(tmp_path_factory):
    return bdlt_ref.build(tmp_path_factory.mktemp("bdlt_oracle"))


@pytest.fixture(scope="module")
def bdl(tmp_path_factory):
    return bdl_ref.build(tmp_path_factory.mktemp("bdlt_oracle_bdl"))


@pytest.fixture(scope="module")
def dirtab(tmp_path_factory):
    return dirtab_ref.build(tmp_path_factory.mktemp("bdlt_oracle_dirtab"))


def _same(got, want, planes=("dirH", "dirI", "dirD")):
    assert (got["score"], got["end"], got["lines"]) == (want["score"], want["end"], want["lines"])
    for key in planes:
        assert np.array_equal(got[key], want[key]), key


@pytest.mark.parametrize("algo", [BSW, BASW])
@pytest.mark.parametrize("alphabet", [2, 26])
def test_an_identity_table_is_match_and_mismatch(bdlt, bdl, algo, alphabet):
    checked = 0
    for wi, w in enumerate(WEIGHTS):
        assert all(-128 <= x <= 127 for x in w[:2])
        table = bdlt_ref.identity_table(w[0], w[1], LETTERS)
        for ref, qry in _pairs(alphabet, 40, 100 * alphabet + 7 * algo + wi):
            for band in BANDS:
                want = bdl.align(algo, ref, qry, w, band, planes=True)
                got = bdlt.align(algo, ref, qry, table, bdl_ref.weights(algo, w)[2:], band, planes=True)
                try:
                    _same(got, want)
                except AssertionError:
                    raise AssertionError((algo, w, band, ref, qry))
                checked += 1
    assert checked == 7 * 47 * 6


def test_basw_at_a_covering_band_is_asw_under_the_table(bdlt, dirtab):
    rng = np.random.default_rng(11)
    for t, table in enumerate((bdlt_ref.dna_table(), bdlt_ref.random_table(3), bdlt_ref.random_table(4, symmetric=True, alphabet=24))):
        for gap in ((-5, -1), (-2, -2), (0, -1), (-11, 0)):
            for ref, qry in _pairs(26, 24, 900 + t):
                if t == 1:  # bytes of the whole range, the upper half included
                    ref, qry = (bytes((x * 37 + 11) & 0xFF for x in s) for s in (ref, qry))
                band = max(len(ref), len(qry), 1) + int(rng.integers(0, 3))
                want = dirtab.align("ASW", ref, qry, table[0], table[1], *gap)
                got = bdlt.align(BASW, ref, qry, table, gap, band, planes=True)
                try:
                    _same(got, want)
                except AssertionError:
                    raise AssertionError((t, gap, band, ref, qry))


# ---- the definition, as a full matrix in plain Python

NEG = -(1 << 60)


def full_matrix(algo, ref, qry, table, g, band):
    """include/dpx_align.h, dpx_batch_set_local_direction_table: the cells with i, j >= 1 and |i - j| <= B - 1; every other cell reads
    H = 0, I = D = -inf; the diagonal term is scores[codeOf[r]][codeOf[q]]"""
    scores, code = table
    n, m = len(ref), len(qry)
    o, e = g
    H = [[0] * (n + 1) for _ in range(m + 1)]
    I = [[NEG] * (n + 1) for _ in range(m + 1)]
    D = [[NEG] * (n + 1) for _ in range(m + 1)]
    dH, dI, dD = (np.zeros((m + 1, n + 1), np.uint8) for _ in range(3))
    t0 = np.zeros((m + 1, n + 1), bool)  # BSW: cells with t == 0
    best, end = 0, (0, 0)
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            if abs(i - j) > band - 1:
                continue
            s = int(scores[code[ref[j - 1]]][code[qry[i - 1]]])
            diag_move = 1 if ref[j - 1] == qry[i - 1] else 2
            corner = H[i - 1][j - 1] + s
            if algo == BASW:
                d_open, d_ext = H[i - 1][j] + o + e, D[i - 1][j] + e
                i_open, i_ext = H[i][j - 1] + o + e, I[i][j - 1] + e
                D[i][j], dD[i, j] = max(d_open, d_ext), 1 if d_open >= d_ext else 2
                I[i][j], dI[i, j] = max(i_open, i_ext), 1 if i_open >= i_ext else 2
                b, mv = corner, diag_move
                if D[i][j] >= b:
                    b, mv = D[i][j], 4
                if I[i][j] >= b:
                    b, mv = I[i][j], 3
                h = max(b, 0)
                dH[i, j] = mv if h else 0
            else:
                up, left = H[i - 1][j] + o, H[i][j - 1] + o
                t = max(up, left, corner)
                h = max(t, 0)
                dH[i, j] = 0 if t < 0 else 4 if up == h else 3 if left == h else diag_move
                t0[i, j] = t == 0
            H[i][j] = h
            if h > best:
                best, end = h, (i, j)
    # the walk: from the end cell in SCORING until H == 0
    lr, lx, lq = bytearray(), bytearray(), bytearray()
    (i, j), state = end, 0
    while i > 0 and j > 0:
        if state == 0:
            if H[i][j] == 0:
                break
            mv = int(dH[i, j])
            if mv in (1, 2):
                lr.append(ref[j - 1]); lx.append(ord("*") if ref[j - 1] == qry[i - 1] else ord("|")); lq.append(qry[i - 1])
                i, j = i - 1, j - 1
                continue
            assert mv in (3, 4)
            if algo == BASW:
                state = 1 if mv == 3 else 2
                continue
            opens = True
        else:
            mv = 3 if state == 1 else 4
            opens = (dI if state == 1 else dD)[i, j] == 1
        if mv == 3:
            lr.append(ref[j - 1]); lx.append(32); lq.append(ord("_"))
            j -= 1
        else:
            lr.append(ord("_")); lx.append(32); lq.append(qry[i - 1])
            i -= 1
        if opens:
            state = 0
    assert state == 0
    return {"score": best, "end": end, "lines": tuple(bytes(reversed(x)) for x in (lr, lx, lq)), "dirH": dH, "dirI": dI, "dirD": dD, "t0": t0}


def _byte_pairs(count, seed):
    """pairs of 0-90 bytes over the whole byte range, half of them related; and the edge cases"""
    rng = np.random.default_rng(seed)
    out = [(b"", b""), (b"", b"\x01\xfe"), (b"\x80", b""), (b"\x07", b"\x07"), (b"\x05" * 40, b"\x05" * 33)]
    for k in range(count):
        n, m = int(rng.integers(0, 91)), int(rng.integers(0, 91))
        ref = rng.integers(0, 256, n).astype(np.uint8)
        if k % 2 and n:
            q = ref.copy()
            sub = rng.random(n) < 0.1
            q[sub] = rng.integers(0, 256, int(sub.sum())).astype(np.uint8)
            q = q[~(rng.random(n) < 0.05)]
            cut = int(rng.integers(0, len(q) + 1))
            q = np.concatenate([q[:cut], rng.integers(0, 256, int(rng.integers(0, 6))).astype(np.uint8), q[cut:]])[:90]
        else:
            q = rng.integers(0, 256, m).astype(np.uint8)
        out.append((ref.tobytes(), q.astype(np.uint8).tobytes()))
    return out


@pytest.mark.parametrize("algo", [BSW, BASW])
def test_asymmetric_tables_at_non_covering_bands_follow_the_definition(bdlt, algo):
    zero_t = past_byte = 0
    for seed in (1, 2):
        table = bdlt_ref.random_table(seed)
        assert table[0].shape == (32, 32) and table[0].min() == -128 and table[0].max() == 127 and not np.array_equal(table[0], table[0].T)
        assert len(set(table[1][128:])) > 1
        g = bdlt_ref.gaps(algo, ((-3, -1), (-7, -2))[seed - 1])
        for ref, qry in _byte_pairs(16, 40 * algo + seed):
            for band in (1, 2, 5, 16, 33):
                want = full_matrix(algo, ref, qry, table, g, band)
                got = bdlt.align(algo, ref, qry, table, g, band, planes=True)
                try:
                    _same(got, want, planes=("dirH",) if algo == BSW else ("dirH", "dirI", "dirD"))
                except AssertionError:
                    raise AssertionError((algo, seed, band, ref, qry))
                zero_t += int(want["t0"].sum())
                past_byte += int(any(x >= 128 for x in ref + qry))
    assert past_byte > 0 and (algo == BASW or zero_t > 0)
