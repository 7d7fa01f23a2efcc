"""The substitution-table oracle (tests/subst_oracle.c) pinned independently of the kernels: (a) hand-computed examples
(tests/golden/subst_examples.json) against the C oracle and the NumPy fill, (b) with scores[a][b] = (a == b ? match : mismatch) and an
injective code map the oracle equals banw_oracle.c / baxt_oracle.c cell for cell and line for line, (c) C against NumPy under random
asymmetric tables, (d) on the ties-and-zeros fuzz set every finite oracle value lies inside the bounds the host's range check derives,
(e) dpx.code_table.  CPU only."""
import json
import os

import numpy as np
import pytest

import banw_ref
import baxt_ref
import subst_ref
from dpx_gpu_genomics_project_amd import code_table

HERE = os.path.dirname(os.path.abspath(__file__))
WEIGHTS = [(3, -1, -3, -1), (2, -3, -5, -1), (1, -4, -2, -1), (3, -2, 0, -2), (1, -1, -3, 2)]


@pytest.fixture(scope="module")
def subst(tmp_path_factory):
    return subst_ref.build(tmp_path_factory.mktemp("subst"))


@pytest.fixture(scope="module")
def baxt(tmp_path_factory):
    return baxt_ref.build(tmp_path_factory.mktemp("baxt_for_subst"))


@pytest.fixture(scope="module")
def banw(tmp_path_factory):
    return banw_ref.build(tmp_path_factory.mktemp("banw_for_subst"))


def _pair(rng, lo=0, hi=14, alphabet=3):
    n, m = int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))
    ref = rng.integers(65, 65 + alphabet, n).astype(np.uint8)
    qry = rng.integers(65, 65 + alphabet, m).astype(np.uint8)
    k = int(rng.integers(0, min(m, n) + 1))
    qry[:k] = ref[:k]
    sub = rng.random(m) < 0.1
    qry[sub] = rng.integers(65, 65 + alphabet, int(sub.sum())).astype(np.uint8)
    return ref.tobytes(), qry.tobytes()


def _numpy_exported(ref, qry, scores, code, o, e, band):
    H, I, D, neg = subst_ref.numpy_fill(ref, qry, scores, code, o, e, band)
    return subst_ref.exported((H, I, D), neg, len(qry), len(ref), band)


def test_a_worked_examples(subst):
    data = json.load(open(os.path.join(HERE, "golden", "subst_examples.json")))
    kinds = {ex["what"] for ex in data["examples"]}
    assert {"asymmetric table", "N against N is no match", "folded case scores as a match and prints a mismatch"} <= kinds, kinds
    for ex in data["examples"]:
        code = code_table(ex["alphabet"].encode(), fold_case=ex["fold_case"])
        scores = np.array(ex["scores"], np.int8)
        ref, qry, (o, e), band, ext = ex["reference"].encode(), ex["query"].encode(), ex["gaps"], ex["band"], ex["algo"] == "BAXT"
        r = subst.align(ref, qry, scores, code, o, e, band, ext)
        assert r["score"] == ex["score"] and list(r["end"]) == ex["end"], (ex["what"], r["score"], r["end"])
        assert [x.decode() for x in r["lines"]] == ex["lines"], ex["what"]
        planes = dict(zip("HID", _numpy_exported(ref, qry, scores, code, o, e, band)))
        for key in "HID":
            if key in ex:
                assert np.array_equal(r[key], np.array(ex[key])), (key, ex["what"], r[key])
                assert np.array_equal(planes[key], np.array(ex[key])), (key, ex["what"], planes[key])
        if "transposed_H11" in ex:  # the row is the reference code: the transposed table is another function
            assert subst.align(ref, qry, scores.T, code, o, e, band, ext)["H"][1, 1] == ex["transposed_H11"] != ex["H"][1][1]
        if "byte_equality_score" in ex:
            ident = subst_ref.identity_table(2, -3, ref + qry)
            assert subst.align(ref, qry, *ident, o, e, band, ext)["score"] == ex["byte_equality_score"] != ex["score"]


def test_b_identity_table_is_plain_scoring(subst, banw, baxt):
    rng = np.random.default_rng(5150)
    compared = {"BANW": 0, "BAXT": 0}
    for k in range(160):
        band = int(rng.integers(1, 7))
        ref, qry = _pair(rng, 0, 12, alphabet=4)
        w = WEIGHTS[k % len(WEIGHTS)]
        scores, code = subst_ref.identity_table(w[0], w[1], ref + qry)
        for name, plain, ext in (("BANW", banw, False), ("BAXT", baxt, True)):
            if not ext and abs(len(ref) - len(qry)) >= band:
                continue
            want = plain.align(ref, qry, *w, band)
            got = subst.align(ref, qry, scores, code, w[2], w[3], band, ext, raw=True)
            assert (got["score"], tuple(got["end"])) == (want["score"], tuple(want["end"])), (name, k)
            for key in ("rawH", "rawI", "rawD", "dirH", "dirI", "dirD", "H", "I", "D"):
                assert np.array_equal(got[key], want[key]), (name, k, key)
            assert got["lines"] == want["lines"], (name, k)
            compared[name] += 1
    assert compared["BANW"] >= 40 and compared["BAXT"] == 160, compared


@pytest.mark.parametrize("alphabet", [1, 2, 5, 24, 32])
def test_c_numpy_fill_agrees_under_random_tables(subst, alphabet):
    rng = np.random.default_rng(900 + alphabet)
    changed = 0
    for k in range(40):
        band = int(rng.integers(1, 8))
        scores = rng.integers(-8, 9, (alphabet, alphabet)).astype(np.int8)
        code = rng.integers(0, alphabet, 256).astype(np.uint8)
        n, m = int(rng.integers(0, 16)), int(rng.integers(0, 16))
        ref, qry = rng.integers(0, 256, n).astype(np.uint8).tobytes(), rng.integers(0, 256, m).astype(np.uint8).tobytes()
        o, e = WEIGHTS[k % len(WEIGHTS)][2:]
        r = subst.align(ref, qry, scores, code, o, e, band, True, raw=True)
        H, I, D, neg = subst_ref.numpy_fill(ref, qry, scores, code, o, e, band)
        for got, want in ((r["rawH"], H), (r["rawI"], I), (r["rawD"], D)):
            assert np.array_equal(np.where(got == subst.neg_inf, neg, got), want), (alphabet, k)
        inb = subst_ref.band_mask(m, n, band)
        assert r["score"] == max(0, int(H[inb].max())) and H[r["end"]] == r["score"], (alphabet, k)
        changed += not np.array_equal(subst.align(ref, qry, scores.T, code, o, e, band, True)["H"], r["H"])
    assert changed >= 1 or alphabet == 1, alphabet  # (a 1 x 1 table is its own transpose)


@pytest.mark.parametrize("table", subst_ref.FUZZ_TABLES)
def test_d_fuzz_set_stays_inside_the_host_bounds(subst, table):
    o, e = subst_ref.FUZZ_GAPS
    code = subst_ref.fuzz_code()
    finite = 0
    for ext in (False, True):
        for band in range(1, 6):
            for ref, qry in subst_ref.fuzz_pairs(band, banw=not ext):
                r = subst.align(ref, qry, table, code, o, e, band, ext, walk=False, raw=True)
                lo, hi = subst_ref.host_bounds(table, o, e, band, len(qry), len(ref))
                assert -32767 <= lo and hi <= 32767
                for key in ("rawH", "rawI", "rawD"):
                    v = r[key][r[key] != subst.neg_inf]
                    finite += v.size
                    assert v.size == 0 or (lo <= v.min() and v.max() <= hi), (table, band, key, lo, hi, v.min(), v.max())
                assert lo <= r["score"] <= hi
    assert finite > 10000


def test_e_code_table():
    dna = code_table(b"ACGTN")
    assert dna.dtype == np.uint8 and dna.shape == (256,)
    assert [int(dna[c]) for c in b"ACGTNacgtn"] == [0, 1, 2, 3, 4, 0, 1, 2, 3, 4]
    assert all(int(dna[x]) == 4 for x in range(256) if x not in b"ACGTacgt")  # every unlisted byte is the last letter
    strict = code_table(b"ACGTN", fold_case=False)
    assert int(strict[ord("a")]) == 4 and int(strict[ord("A")]) == 0
    both = code_table(b"Aa")  # a listed lower-case letter keeps its own code
    assert (int(both[ord("A")]), int(both[ord("a")])) == (0, 1)
    for bad in (b"", b"AA", bytes(range(33))):
        with pytest.raises(ValueError):
            code_table(bad)
