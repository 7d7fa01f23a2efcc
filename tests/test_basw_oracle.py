"""The banded affine-gap Smith-Waterman oracle (tests/basw_oracle.c) against the definition in include/dpx_align.h: a covering band is
ASW (tests/asw_oracle.c), gapOpen = 0 is the banded linear-gap oracle, a plain-Python per-cell model, the score and the band membership
of every printed path, and the worked examples of tests/golden/basw_examples.json.  CPU only."""
import json
import os

import numpy as np
import pytest

import asw_ref
import basw_ref
import oracle_py as O

HERE = os.path.dirname(os.path.abspath(__file__))
WEIGHTS = [(3, -1, -3, -1), (2, -3, -5, -2), (3, -1, 2, -3), (3, -2, -4, 1)]  # both signs, o + e > 0 among them


@pytest.fixture(scope="module")
def basw(tmp_path_factory):
    return basw_ref.build(tmp_path_factory.mktemp("basw"))


@pytest.fixture(scope="module")
def asw(tmp_path_factory):
    return asw_ref.build(tmp_path_factory.mktemp("basw_asw"))


def _related(rng, lo=0, hi=60, alphabet=4):
    """a query that is a mutated window of its reference at an offset (so that a narrow band loses part of the alignment)"""
    n, m = int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))
    ref = rng.integers(65, 65 + alphabet, n).astype(np.uint8)
    start = int(rng.integers(0, max(n - m, 0) + 1))
    q = ref[start:start + m].copy()
    q = np.concatenate([q, rng.integers(65, 65 + alphabet, m - len(q)).astype(np.uint8)])
    sub = rng.random(m) < 0.12
    q[sub] = rng.integers(65, 65 + alphabet, int(sub.sum())).astype(np.uint8)
    q = q[~(rng.random(m) < 0.04)]
    return ref.tobytes(), q.astype(np.uint8).tobytes()


def _model(ref, qry, match, mismatch, o, e, B):
    """the definition, cell by cell, in plain Python: out-of-band and border neighbours read H = 0, I = D = -inf"""
    n, m = len(ref), len(qry)
    NEG = float("-inf")
    inb = lambda i, j: i >= 1 and j >= 1 and abs(i - j) <= B - 1
    H, I, D = {}, {}, {}
    h = lambda i, j: H[i, j] if inb(i, j) else 0
    best, end = 0, (0, 0)
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            if not inb(i, j):
                continue
            D[i, j] = max(h(i - 1, j) + o + e, (D[i - 1, j] if inb(i - 1, j) else NEG) + e)
            I[i, j] = max(h(i, j - 1) + o + e, (I[i, j - 1] if inb(i, j - 1) else NEG) + e)
            b = h(i - 1, j - 1) + (match if qry[i - 1] == ref[j - 1] else mismatch)
            if D[i, j] >= b:
                b = D[i, j]
            if I[i, j] >= b:
                b = I[i, j]
            H[i, j] = max(0, b)
            if H[i, j] > best:
                best, end = H[i, j], (i, j)
    out = [np.zeros((m + 1, n + 1), np.int64) for _ in range(3)]
    for k, M in enumerate((H, I, D)):
        for (i, j), v in M.items():
            out[k][i, j] = v
    return out, best, end


def test_oracle_matches_python_model(basw):
    rng = np.random.default_rng(101)
    lowered = 0
    for k in range(200):
        ref, qry = _related(rng, 0, 40)
        w = WEIGHTS[k % 4] if k % 2 else tuple(int(rng.integers(-6, 7)) for _ in range(4))
        B = int(rng.integers(1, 24))
        (H, I, D), best, end = _model(ref, qry, *w, B)
        r = basw.align(ref, qry, *w, B)
        assert np.array_equal(r["H"], H) and np.array_equal(r["I"], I) and np.array_equal(r["D"], D), (k, ref, qry, w, B)
        assert (r["score"], r["end"]) == (best, end), (k, ref, qry, w, B)
        lowered += best < _model(ref, qry, *w, max(len(ref), len(qry), 1))[1]
    assert lowered >= 10, lowered  # the band mattered


def test_covering_band_is_asw(basw, asw):
    """identity (a): B >= max(m, n) gives ASW's matrices, enums, end cell and lines"""
    rng = np.random.default_rng(102)
    for k in range(200):
        ref, qry = _related(rng)
        w = WEIGHTS[k % 4]
        B = max(len(ref), len(qry), 1) + int(rng.integers(0, 3))
        r, a = basw.align(ref, qry, *w, B), asw.align(ref, qry, *w)
        for key in ("H", "I", "D", "dirH", "dirI", "dirD"):
            assert np.array_equal(r[key], a[key]), (k, key, ref, qry, w, B)
        assert (r["score"], r["end"], r["lines"]) == (a["score"], a["end"], a["lines"]), (k, ref, qry, w, B)


def test_open_zero_is_the_banded_linear_oracle(basw):
    """identity (b): gapOpen = 0 gives BSW's H, score and end cell with linear gap gapExtend and the same band"""
    rng = np.random.default_rng(103)
    for k in range(200):
        ref, qry = _related(rng)
        match, mismatch, g = int(rng.integers(-2, 6)), int(rng.integers(-6, 3)), int(rng.integers(-5, 3))
        B = int(rng.integers(1, 24))
        r = basw.align(ref, qry, match, mismatch, 0, g, B)
        l = O.lsw(ref, qry, match, mismatch, g, band=B, want_dir=False)
        assert np.array_equal(r["H"], l.H), (k, ref, qry, match, mismatch, g, B)
        assert (r["score"], r["end"]) == (l.score, (l.end_row, l.end_col)), (k, ref, qry, match, mismatch, g, B)


def _rescore(ref, qry, r, match, mismatch, o, e, B):
    """walk the printed lines back from the end cell: every step inside the band, each gap run worth o + L * e; returns the path's score"""
    lr, lx, lq = r["lines"]
    i, j = r["end"]
    total, kind = 0, None
    for a, x, b in zip(reversed(lr), reversed(lx), reversed(lq)):
        assert 1 <= i <= len(qry) and 1 <= j <= len(ref) and abs(i - j) <= B - 1, (i, j, B)
        if x in (ord("*"), ord("|")):
            assert a == ref[j - 1] and b == qry[i - 1] and (a == b) == (x == ord("*"))
            total += match if a == b else mismatch
            kind = None
            i, j = i - 1, j - 1
        elif b == ord("_"):
            assert a == ref[j - 1] and x == ord(" ")
            total += e if kind == "I" else o + e
            kind = "I"
            j -= 1
        else:
            assert a == ord("_") and b == qry[i - 1] and x == ord(" ")
            total += e if kind == "D" else o + e
            kind = "D"
            i -= 1
    return total


def test_printed_paths_rescore_and_stay_in_the_band(basw):
    """non-positive gap weights: every printed alignment is an in-band path worth exactly the reported score"""
    rng = np.random.default_rng(104)
    gaps = 0
    for k in range(300):
        ref, qry = _related(rng)
        w = (int(rng.integers(1, 6)), int(rng.integers(-6, 1)), int(rng.integers(-6, 1)), int(rng.integers(-4, 1)))
        B = int(rng.integers(1, 24))
        r = basw.align(ref, qry, *w, B)
        assert _rescore(ref, qry, r, *w, B) == r["score"], (k, ref, qry, w, B, r["lines"])
        gaps += b"_" in r["lines"][0] or b"_" in r["lines"][2]
        if r["score"] == 0:
            assert r["lines"] == (b"", b"", b"") and r["end"] == (0, 0)
    assert gaps >= 20, gaps


def test_worked_examples(basw):
    data = json.load(open(os.path.join(HERE, "golden", "basw_examples.json")))
    assert len(data["examples"]) >= 5
    for ex in data["examples"]:
        r = basw.align(ex["reference"].encode(), ex["query"].encode(), *ex["weights"], ex["band"])
        assert r["score"] == ex["score"], ex
        assert list(r["end"]) == ex["end"], ex
        assert [x.decode() for x in r["lines"]] == ex["lines"], ex
        for key in ("H", "I", "D"):
            if key in ex:
                assert np.array_equal(r[key], np.array(ex[key])), (key, ex)
