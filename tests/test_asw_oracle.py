"""The affine-gap Smith-Waterman oracle (tests/asw_oracle.c) against the definition: the worked examples of
tests/golden/asw_examples.json, a plain-Python per-cell model, the LSW oracle at gapOpen = 0, and the score of every printed path.
CPU only."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import asw_ref
import oracle_py as O

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def asw(tmp_path_factory):
    return asw_ref.build(tmp_path_factory.mktemp("asw"))


def _model(ref, qry, match, mismatch, o, e):
    """the definition, cell by cell, in plain Python"""
    n, m = len(ref), len(qry)
    NEG = float("-inf")
    H = [[0] * (n + 1) for _ in range(m + 1)]
    I = [[NEG] * (n + 1) for _ in range(m + 1)]
    D = [[NEG] * (n + 1) for _ in range(m + 1)]
    best, end = 0, (0, 0)
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            D[i][j] = max(H[i - 1][j] + o + e, D[i - 1][j] + e)
            I[i][j] = max(H[i][j - 1] + o + e, I[i][j - 1] + e)
            b = H[i - 1][j - 1] + (match if qry[i - 1] == ref[j - 1] else mismatch)
            if D[i][j] >= b:
                b = D[i][j]
            if I[i][j] >= b:
                b = I[i][j]
            H[i][j] = max(0, b)
            if H[i][j] > best:
                best, end = H[i][j], (i, j)
    return np.array(H), best, end


def _rand(rng, alphabet=4):
    n, m = int(rng.integers(0, 41)), int(rng.integers(0, 41))
    return rng.integers(65, 65 + alphabet, n).astype(np.uint8).tobytes(), rng.integers(65, 65 + alphabet, m).astype(np.uint8).tobytes()


def test_worked_examples(asw):
    data = json.load(open(os.path.join(HERE, "golden", "asw_examples.json")))
    for ex in data["examples"]:
        r = asw.align(ex["reference"].encode(), ex["query"].encode(), *ex["weights"])
        assert r["score"] == ex["score"], ex
        assert list(r["end"]) == ex["end"], ex
        assert [x.decode() for x in r["lines"]] == ex["lines"], ex
        if "H" in ex:
            assert np.array_equal(r["H"], np.array(ex["H"])), ex
        if "I_interior" in ex:
            assert (r["I"][1:, 1:] == ex["I_interior"]).all() and (r["D"][1:, 1:] == ex["D_interior"]).all()
            assert not r["I"][0].any() and not r["I"][:, 0].any() and not r["D"][0].any() and not r["D"][:, 0].any()


def test_oracle_matches_python_model(asw):
    rng = np.random.default_rng(11)
    o = asw
    for k in range(200):
        ref, qry = _rand(rng)
        w = [int(rng.integers(-6, 7)) for _ in range(4)]
        H, best, end = _model(ref, qry, *w)
        r = o.align(ref, qry, *w)
        assert np.array_equal(r["H"], H), (k, ref, qry, w)
        assert (r["score"], r["end"]) == (best, end), (k, ref, qry, w)


def test_open_zero_equals_lsw_oracle(asw):
    """gapOpen = 0: ASW's H, score and end cell are LSW's with gap = gapExtend (the reference-pinned LSW oracle)"""
    orc = O.oracle()
    rng = np.random.default_rng(12)
    for k in range(300):
        ref, qry = _rand(rng)
        match, mismatch, g = int(rng.integers(-2, 6)), int(rng.integers(-6, 3)), int(rng.integers(-5, 3))
        r = asw.align(ref, qry, match, mismatch, 0, g)
        n, m = len(ref), len(qry)
        H = np.zeros((m + 1, n + 1), np.int32)
        sc, er, ec = C.c_int32(), C.c_int32(), C.c_int32()
        orc.orc_lsw_fill(ref, n, qry, m, match, mismatch, g, H.ctypes.data, None, C.addressof(sc), C.addressof(er), C.addressof(ec))
        assert np.array_equal(r["H"], H), (k, ref, qry, match, mismatch, g)
        assert (r["score"], r["end"]) == (sc.value, (er.value, ec.value)), (k, ref, qry, match, mismatch, g)


def _path_score(lines, match, mismatch, o, e):
    lr, lx, lq = lines
    total, run, kind = 0, 0, None
    for a, x, b in zip(lr, lx, lq):
        if x in (ord("*"), ord("|")):
            assert (a == b) == (x == ord("*"))
            total += match if a == b else mismatch
            kind = None
        else:
            k = "I" if b == ord("_") else "D"
            total += (o + e) if k != kind else e
            kind = k
    return total


def test_printed_paths_score_the_reported_score(asw):
    """non-positive gap weights: every printed alignment is a path worth exactly the score (each gap run o + L * e)"""
    rng = np.random.default_rng(13)
    for k in range(300):
        ref, qry = _rand(rng)
        w = (int(rng.integers(1, 6)), int(rng.integers(-6, 1)), int(rng.integers(-6, 1)), int(rng.integers(-4, 1)))
        r = asw.align(ref, qry, *w)
        assert _path_score(r["lines"], *w) == r["score"], (k, ref, qry, w, r["lines"])
        if r["score"] == 0:
            assert r["lines"] == (b"", b"", b"") and r["end"] == (0, 0)
