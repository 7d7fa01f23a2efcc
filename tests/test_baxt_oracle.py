"""The banded affine-gap extension oracle (tests/baxt_oracle.c) against the definition in include/dpx_align.h, pinned independently of
the kernels: (a) worked examples small enough to check by hand (tests/golden/baxt_examples.json), (b) the score identity
BAXT(ref, qry, B) = max over in-band (i, j) of BANW(ref[:j], qry[:i], B) against the BANW oracle, with the first row-major maximum as
the end cell, (c) H / I / D equal BANW's raw planes wherever BANW admits the pair, (d) a score of 0 ends at (0, 0), (e) the printed
path rescores to the score, its ungapped characters are ref[:endCol] / qry[:endRow], and every walked cell is in the band.  CPU only."""
import json
import os

import numpy as np
import pytest

import banw_ref
import baxt_ref

HERE = os.path.dirname(os.path.abspath(__file__))
WEIGHTS = [(3, -1, -3, -1), (2, -3, -5, -1), (1, -4, -2, -1), (3, -2, 0, -2), (1, -1, -3, 2)]


@pytest.fixture(scope="module")
def baxt(tmp_path_factory):
    return baxt_ref.build(tmp_path_factory.mktemp("baxt"))


@pytest.fixture(scope="module")
def banw(tmp_path_factory):
    return banw_ref.build(tmp_path_factory.mktemp("banw_for_baxt"))


def _pair(rng, lo=0, hi=14, alphabet=3):
    """a query that starts as a mutated copy of the reference's start; any two lengths"""
    n, m = int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))
    ref = rng.integers(65, 65 + alphabet, n).astype(np.uint8)
    qry = rng.integers(65, 65 + alphabet, m).astype(np.uint8)
    k = int(rng.integers(0, min(m, n) + 1))
    qry[:k] = ref[:k]
    sub = rng.random(m) < 0.1
    qry[sub] = rng.integers(65, 65 + alphabet, int(sub.sum())).astype(np.uint8)
    return ref.tobytes(), qry.tobytes()


def test_a_worked_examples(baxt):
    data = json.load(open(os.path.join(HERE, "golden", "baxt_examples.json")))
    kinds = {ex["what"] for ex in data["examples"]}
    assert {"B = 1", "score 0", "border end", "m = 0, border end", "n = 0", "end inside the matrix, |m - n| >= B"} <= kinds, kinds
    for ex in data["examples"]:
        r = baxt.align(ex["reference"].encode(), ex["query"].encode(), *ex["weights"], ex["band"])
        assert r["score"] == ex["score"] and list(r["end"]) == ex["end"], (ex, r["score"], r["end"])
        assert [x.decode() for x in r["lines"]] == ex["lines"], ex
        for key in ("H", "I", "D"):
            if key in ex:
                assert np.array_equal(r[key], np.array(ex[key])), (key, ex, r[key])


def test_b_score_is_the_best_banw_score_over_in_band_prefixes(baxt, banw):
    rng = np.random.default_rng(301)
    inside = 0
    for k in range(120):
        B = int(rng.integers(1, 7))
        ref, qry = _pair(rng, 0, 11)
        w = WEIGHTS[k % len(WEIGHTS)]
        best, at = None, None
        for i in range(len(qry) + 1):  # row-major: the first maximum wins
            for j in range(len(ref) + 1):
                if abs(i - j) <= B - 1:
                    sc = banw.score(ref[:j], qry[:i], w, B)
                    if best is None or sc > best:
                        best, at = sc, (i, j)
        got = baxt.result(ref, qry, w, B)
        assert got == (best, *at), (k, ref, qry, w, B, got, best, at)
        assert got[0] >= 0
        inside += at not in ((0, 0), (len(qry), len(ref)))
    assert inside >= 20, inside


def test_c_cells_are_banw_cells_where_banw_admits(baxt, banw):
    rng = np.random.default_rng(302)
    admitted = 0
    for k in range(200):
        B = int(rng.integers(1, 9))
        ref, qry = _pair(rng, 0, 16)
        w = WEIGHTS[k % len(WEIGHTS)]
        if not banw.admits(ref, qry, B):
            continue
        admitted += 1
        a, b = baxt.align(ref, qry, *w, B, walk=False), banw.align(ref, qry, *w, B, walk=False)
        assert baxt.neg_inf == banw.neg_inf
        for key in ("rawH", "rawI", "rawD", "dirH", "dirI", "dirD"):
            assert np.array_equal(a[key], b[key]), (k, key, ref, qry, w, B)
        assert a["score"] >= b["score"]
    assert admitted >= 60, admitted


def test_d_score_zero_ends_at_the_anchor_and_the_maximum_is_the_first(baxt):
    rng = np.random.default_rng(303)
    zeros = ties = 0
    for k in range(300):
        B = int(rng.integers(1, 6))
        ref, qry = _pair(rng, 0, 13, alphabet=2)
        w = WEIGHTS[k % len(WEIGHTS)]
        r = baxt.align(ref, qry, *w, B)
        inb = baxt_ref.band_mask(len(qry), len(ref), B)
        H = np.where(inb, r["rawH"], baxt.neg_inf)
        assert r["score"] == H.max() >= 0
        flat = np.flatnonzero(H.ravel() == r["score"])
        assert r["end"] == divmod(int(flat[0]), len(ref) + 1), (k, ref, qry, w, B)
        ties += len(flat) > 1
        if r["score"] == 0:
            zeros += 1
            assert r["end"] == (0, 0) and r["lines"] == (b"", b"", b"")
    assert zeros >= 20 and ties >= 20, (zeros, ties)


def _rescore(ref, qry, lines, match, mismatch, o, e, B):
    """walk the printed lines forward from (0, 0): every cell inside the band, each gap run worth o + L * e; returns score and end cell"""
    i = j = total = 0
    kind = None
    for a, x, b in zip(*lines):
        if x in (ord("*"), ord("|")):
            assert a == ref[j] and b == qry[i] and (a == b) == (x == ord("*"))
            total += match if a == b else mismatch
            kind = None
            i, j = i + 1, j + 1
        elif b == ord("_"):
            assert a == ref[j] and x == ord(" ")
            total += e if kind == "I" else o + e
            kind = "I"
            j += 1
        else:
            assert a == ord("_") and b == qry[i] and x == ord(" ")
            total += e if kind == "D" else o + e
            kind = "D"
            i += 1
        assert abs(i - j) <= B - 1, (i, j, B)
    return total, (i, j)


def test_e_printed_paths_rescore_reach_the_anchor_and_stay_in_the_band(baxt):
    rng = np.random.default_rng(304)
    gaps = inside = 0
    for k in range(300):
        B = int(rng.integers(1, 12))
        ref, qry = _pair(rng, 0, 40, alphabet=4)
        w = (int(rng.integers(1, 6)), int(rng.integers(-6, 1)), int(rng.integers(-6, 1)), int(rng.integers(-4, 1))) if k % 3 else WEIGHTS[4]
        r = baxt.align(ref, qry, *w, B)
        er, ec = r["end"]
        assert _rescore(ref, qry, r["lines"], *w, B) == (r["score"], (er, ec)), (k, ref, qry, w, B, r["lines"])
        assert r["lines"][0].replace(b"_", b"") == ref[:ec] and r["lines"][2].replace(b"_", b"") == qry[:er]
        assert r["cells"][0] == (er, ec) and r["cells"][-1] == (0, 0)
        assert all(abs(i - j) <= B - 1 for i, j in r["cells"])
        assert len(r["cells"]) == len(r["lines"][0]) + 1
        gaps += b"_" in r["lines"][0] or b"_" in r["lines"][2]
        inside += (er, ec) not in ((0, 0), (len(qry), len(ref)))
    assert gaps >= 20 and inside >= 20, (gaps, inside)
