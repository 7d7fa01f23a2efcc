"""The banded affine-gap Needleman-Wunsch oracle (tests/banw_oracle.c) against the definition in include/dpx_align.h, pinned six ways:
(a) worked examples small enough to check by hand (tests/golden/banw_examples.json), (b) a plain-Python per-cell model, (c) brute force
over every in-band path of tiny inputs, (d) a covering band is the project's ANW oracle and B = max(m, n) differs from it exactly where
the definition says, (e) the score grows with the band up to ANW's, (f) the printed lines rescore to the score on a path inside the
band.  CPU only."""
import itertools
import json
import os

import numpy as np
import pytest

import banw_ref
import oracle_py as O

HERE = os.path.dirname(os.path.abspath(__file__))
WEIGHTS = [(3, -1, -3, -1), (2, -3, -5, -1), (1, -4, -2, -1), (3, -2, 0, -2)]
NEG = float("-inf")


@pytest.fixture(scope="module")
def banw(tmp_path_factory):
    return banw_ref.build(tmp_path_factory.mktemp("banw"))


def _pair(rng, band, lo=0, hi=40, alphabet=4):
    """a query that is a mutated copy of its reference, lengths within the band's reach of each other"""
    n = int(rng.integers(lo, hi + 1))
    ref = rng.integers(65, 65 + alphabet, n).astype(np.uint8)
    q = ref.copy()
    sub = rng.random(n) < 0.12
    q[sub] = rng.integers(65, 65 + alphabet, int(sub.sum())).astype(np.uint8)
    q = q[~(rng.random(n) < 0.06)]
    ins = rng.integers(65, 65 + alphabet, int(rng.integers(0, 4))).astype(np.uint8)
    at = int(rng.integers(0, len(q) + 1))
    q = np.concatenate([q[:at], ins, q[at:]])
    while abs(len(q) - n) > band - 1:  # the admission rule: trim the longer one
        if len(q) > n:
            q = q[:-1]
        else:
            ref, n = ref[:-1], n - 1
    return ref.tobytes(), q.astype(np.uint8).tobytes()


def _model(ref, qry, match, mismatch, o, e, B):
    """the definition, cell by cell, in plain Python with float -inf"""
    n, m = len(ref), len(qry)
    inb = lambda i, j: abs(i - j) <= B - 1
    H = {(i, j): NEG for i in range(-1, m + 1) for j in range(-1, n + 1)}
    I, D = dict(H), dict(H)
    H[0, 0] = 0
    for i in range(1, m + 1):
        if inb(i, 0):
            H[i, 0] = o + i * e
    for j in range(1, n + 1):
        if inb(0, j):
            H[0, j] = o + j * e
    for i in range(1, m + 1):
        for j in range(1, n + 1):
            if not inb(i, j):
                continue
            D[i, j] = max(H[i - 1, j] + o + e, D[i - 1, j] + e)
            I[i, j] = max(H[i, j - 1] + o + e, I[i, j - 1] + e)
            H[i, j] = max(H[i - 1, j - 1] + (match if qry[i - 1] == ref[j - 1] else mismatch), D[i, j], I[i, j])
    return H, I, D


def test_b_oracle_matches_python_model(banw):
    rng = np.random.default_rng(201)
    for k in range(200):
        B = int(rng.integers(1, 12))
        ref, qry = _pair(rng, B, 0, 24)
        w = WEIGHTS[k % 4] if k % 2 else tuple(int(rng.integers(-6, 7)) for _ in range(4))
        H, I, D = _model(ref, qry, *w, B)
        r = banw.align(ref, qry, *w, B)
        for name, M in (("rawH", H), ("rawI", I), ("rawD", D)):
            for i in range(len(qry) + 1):
                for j in range(len(ref) + 1):
                    got = r[name][i, j]
                    assert (NEG if got == banw.neg_inf else got) == M[i, j], (k, name, i, j, ref, qry, w, B)
        assert r["score"] == H[len(qry), len(ref)]
        # what follows from the rule: in-band H finite; I on the lower edge and D on the upper edge are -infinity, and nothing else in band is
        inb = banw_ref.band_mask(len(qry), len(ref), B)
        i, j = np.mgrid[0:len(qry) + 1, 0:len(ref) + 1]
        inner = inb & (i >= 1) & (j >= 1)
        assert np.all((r["rawH"] != banw.neg_inf) == inb)
        assert np.array_equal((r["rawI"] == banw.neg_inf) & inner, inner & (i - j == B - 1))
        assert np.array_equal((r["rawD"] == banw.neg_inf) & inner, inner & (j - i == B - 1))


def _paths(m, n, B):
    """every monotone path (0, 0) -> (m, n) whose cells all satisfy |i - j| <= B - 1, as strings of 'M' (diagonal), 'D' (up), 'I' (left)"""
    def go(i, j):
        if abs(i - j) > B - 1:
            return
        if (i, j) == (m, n):
            yield ""
            return
        if i < m and j < n:
            for t in go(i + 1, j + 1):
                yield "M" + t
        if i < m:
            for t in go(i + 1, j):
                yield "D" + t
        if j < n:
            for t in go(i, j + 1):
                yield "I" + t
    return go(0, 0)


def _path_score(path, ref, qry, match, mismatch, o, e):
    i = j = total = 0
    prev = None
    for s in path:
        if s == "M":
            total += match if qry[i] == ref[j] else mismatch
            i, j = i + 1, j + 1
        else:
            total += e if prev == s else o + e
            if s == "D":
                i += 1
            else:
                j += 1
        prev = s
    return total


def test_c_brute_force_over_every_in_band_path(banw):
    rng = np.random.default_rng(202)
    checked = 0
    for m, n in itertools.product(range(6), range(6)):
        for B in range(abs(m - n) + 1, max(m, n) + 3):
            for w in ((3, -1, -3, -1), (1, -4, -2, -1), (2, -3, 0, -2)):
                ref = rng.integers(65, 67, n).astype(np.uint8).tobytes()
                qry = rng.integers(65, 67, m).astype(np.uint8).tobytes()
                best = max(_path_score(p, ref, qry, *w) for p in _paths(m, n, B))
                assert banw.score(ref, qry, w, B) == best, (ref, qry, w, B)
                checked += 1
    assert checked > 300
    assert not banw.admits(b"AAAA", b"A", 3) and banw.admits(b"AAAA", b"A", 4)  # |m - n| >= B: no path


def test_d_covering_band_is_anw_and_one_less_is_not(banw):
    rng = np.random.default_rng(203)
    differed = 0
    for k in range(150):
        ref, qry = _pair(rng, 1000, 0, 30)
        w = WEIGHTS[k % 4]
        n, m = len(ref), len(qry)
        a = O.anw(ref, qry, *w)
        r = banw.align(ref, qry, *w, max(m, n) + 1 + int(rng.integers(0, 3)))
        for key in ("H", "I", "D"):
            assert np.array_equal(r[key], getattr(a, key)), (k, key, ref, qry, w)
        assert r["score"] == a.score
        assert tuple(x.decode("latin-1") for x in r["lines"]) == O.anw_traceback(ref, qry, a), (k, ref, qry, w)
        # B = max(m, n): only the corner border cells (m, 0) / (0, n) leave the band, and with them the I of row m's / the D of column n's
        # in-band cells can only fall; every cell whose paths avoid the corner keeps its value
        B = max(m, n)
        if B >= 1 and abs(m - n) <= B - 1:
            s = banw.align(ref, qry, *w, B)
            inb = banw_ref.band_mask(m, n, B)
            assert np.array_equal(~inb, (np.mgrid[0:m + 1, 0:n + 1][0] - np.mgrid[0:m + 1, 0:n + 1][1] == B) |
                                  (np.mgrid[0:m + 1, 0:n + 1][1] - np.mgrid[0:m + 1, 0:n + 1][0] == B))
            for key in ("rawH", "rawI", "rawD"):
                lower = np.where(s[key] == banw.neg_inf, -10**9, s[key]) <= np.where(r[key] == banw.neg_inf, -10**9, r[key])
                assert np.all(lower), (k, key)
            same = np.ones((m + 1, n + 1), bool)
            if m == B:
                same[m, :] = False  # row m can reach (m, 0)
            if n == B:
                same[:, n] = False
            for key in ("rawH", "rawI", "rawD"):
                assert np.array_equal(s[key][same], r[key][same]), (k, key, ref, qry, w)
            if m == B and n >= 1:
                assert s["rawI"][m, 1] == banw.neg_inf and r["rawI"][m, 1] == w[2] + m * w[3] + w[2] + w[3]
                differed += 1
    assert differed >= 20
    # the example of the definition: ACGTAC / AGTTAC, 3 / -1 / -3 / -1
    full, cut = banw.align(b"ACGTAC", b"AGTTAC", 3, -1, -3, -1, 7), banw.align(b"ACGTAC", b"AGTTAC", 3, -1, -3, -1, 6)
    assert full["rawI"][6, 1] == -13 == O.anw(b"ACGTAC", b"AGTTAC", 3, -1, -3, -1).I[6, 1] and cut["rawI"][6, 1] == banw.neg_inf


def test_e_score_grows_with_the_band_up_to_anw(banw):
    rng = np.random.default_rng(204)
    strict = 0
    for k in range(150):
        ref, qry = _pair(rng, 3, 0, 40)
        w = WEIGHTS[k % 4]
        anw = O.anw(ref, qry, *w, want_dir=False).score
        prev = None
        for B in range(abs(len(ref) - len(qry)) + 1, max(len(ref), len(qry)) + 3):
            sc = banw.score(ref, qry, w, B)
            assert sc <= anw and (prev is None or prev <= sc), (k, B, ref, qry, w)
            strict += prev is not None and prev < sc
            prev = sc
        assert prev == anw
    assert strict >= 50, strict


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


def test_f_printed_paths_rescore_and_stay_in_the_band(banw):
    rng = np.random.default_rng(205)
    gaps = negative = 0
    for k in range(300):
        B = int(rng.integers(1, 12))
        ref, qry = _pair(rng, B)
        w = (int(rng.integers(1, 6)), int(rng.integers(-6, 1)), int(rng.integers(-6, 1)), int(rng.integers(-4, 1)))
        r = banw.align(ref, qry, *w, B)
        assert _rescore(ref, qry, r["lines"], *w, B) == (r["score"], (len(qry), len(ref))), (k, ref, qry, w, B, r["lines"])
        gaps += b"_" in r["lines"][0] or b"_" in r["lines"][2]
        negative += r["score"] < 0
    assert gaps >= 20 and negative >= 5, (gaps, negative)


def test_a_worked_examples(banw):
    data = json.load(open(os.path.join(HERE, "golden", "banw_examples.json")))
    kinds = {ex["what"] for ex in data["examples"]}
    assert {"B = 1", "corner on the band's edge", "m = 0", "negative score"} <= kinds, kinds
    for ex in data["examples"]:
        r = banw.align(ex["reference"].encode(), ex["query"].encode(), *ex["weights"], ex["band"])
        assert r["score"] == ex["score"], ex
        assert [x.decode() for x in r["lines"]] == ex["lines"], ex
        for key in ("H", "I", "D"):
            assert np.array_equal(r[key], np.array(ex[key])), (key, ex)
