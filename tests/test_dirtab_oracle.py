"""The oracle of ANW / ASW / ASG under a substitution table (tests/dirtab_oracle.c) pinned three independent ways: under the table that
scores as byte equality does it equals the ASW, ASG and ANW oracles (score, end cell, enum planes, lines); ANW under random asymmetric
tables equals tests/subst_oracle.c in BANW mode under the covering band max(m, n) + 1; ASW / ASG scores and end cells equal an
anti-diagonal NumPy fill written for this test (dirtab_ref.numpy_result).  CPU only."""
import numpy as np
import pytest

import asg_ref
import asw_ref
import dirtab_ref
import oracle_py as O
import subst_ref


@pytest.fixture(scope="module")
def dt(tmp_path_factory):
    return dirtab_ref.build(tmp_path_factory.mktemp("dirtab"))


@pytest.fixture(scope="module")
def others(tmp_path_factory):
    d = tmp_path_factory.mktemp("dirtab_others")
    return {"ASW": asw_ref.build(d), "ASG": asg_ref.build(d), "subst": subst_ref.build(d)}


def _pairs(seed, letters=4):
    """300 pairs with m, n in 0..40 and a handful up to 300"""
    rng = np.random.default_rng(seed)
    sizes = [(int(rng.integers(0, 41)), int(rng.integers(0, 41))) for _ in range(300)] + [(300, 280), (257, 300), (129, 64), (1, 300), (300, 0)]
    return rng, [(rng.integers(65, 65 + letters, n).astype(np.uint8).tobytes(), rng.integers(65, 65 + letters, m).astype(np.uint8).tobytes())
                 for n, m in sizes]


def test_identity_table_equals_the_three_plain_oracles(dt, others):
    rng, pairs = _pairs(1)
    for k, (ref, qry) in enumerate(pairs):
        w = [int(rng.integers(-6, 7)) for _ in range(4)]
        tab, code = subst_ref.identity_table(w[0], w[1], ref + qry)
        for kind in ("ASW", "ASG"):
            want = others[kind].align(ref, qry, *w)
            got = dt.align(kind, ref, qry, tab, code, w[2], w[3])
            assert (got["score"], got["end"], got["lines"]) == (want["score"], want["end"], want["lines"]), (kind, k, ref, qry, w)
            for key in ("dirH", "dirI", "dirD"):
                assert np.array_equal(got[key], want[key]), (kind, key, k, ref, qry, w)
        want = O.anw(ref, qry, *w)
        got = dt.align("ANW", ref, qry, tab, code, w[2], w[3])
        assert (got["score"], got["end"]) == (want.score, (len(qry), len(ref))), (k, ref, qry, w)
        assert got["lines"] == tuple(x.encode("latin-1") for x in O.anw_traceback(ref, qry, want)), (k, ref, qry, w)
        for key in ("dirH", "dirI", "dirD"):
            assert np.array_equal(got[key], getattr(want, key)), (key, k, ref, qry, w)


def test_anw_under_asymmetric_tables_equals_the_covering_band(dt, others):
    rng, pairs = _pairs(2, letters=6)
    for k, (ref, qry) in enumerate(pairs):
        tab, code = dirtab_ref.random_table(rng, int(rng.integers(1, 8)))
        o, e = int(rng.integers(-6, 3)), int(rng.integers(-4, 2))
        band = max(len(ref), len(qry)) + 1
        want = others["subst"].align(ref, qry, tab, code, o, e, band, False)
        got = dt.align("ANW", ref, qry, tab, code, o, e)
        assert (got["score"], got["end"], got["lines"]) == (want["score"], want["end"], want["lines"]), (k, ref, qry, tab.tolist(), o, e)
        for key in ("dirH", "dirI", "dirD"):  # (the cells: subst_oracle.c leaves the border enums to the export; the identity test pins them)
            assert np.array_equal(got[key][1:, 1:], want[key][1:, 1:]), (key, k, ref, qry, o, e)


def test_asw_and_asg_equal_the_numpy_fill(dt):
    rng, pairs = _pairs(3, letters=6)
    transposed_differs = 0
    for k, (ref, qry) in enumerate(pairs):
        tab, code = dirtab_ref.random_table(rng, int(rng.integers(1, 8)))
        o, e = int(rng.integers(-6, 3)), int(rng.integers(-4, 2))
        for kind in ("ASW", "ASG", "ANW"):
            got = dt.align(kind, ref, qry, tab, code, o, e)
            assert (got["score"], got["end"]) == dirtab_ref.numpy_result(kind, ref, qry, tab, code, o, e), (kind, k, ref, qry, tab.tolist(), o, e)
            transposed_differs += got["score"] != dt.align(kind, ref, qry, tab.T.copy(), code, o, e)["score"]
    assert transposed_differs > 300  # the row of the table is the reference code, and these tables say so


def test_text_is_byte_equality_and_empty_sequences(dt):
    tab = np.array([[2, -1], [-1, -3]], np.int8)  # code 1 against code 1 scores -3
    code = np.zeros(256, np.uint8)
    code[ord("N")] = code[ord("n")] = 1
    code[ord("a")] = 0
    r = dt.align("ANW", b"AaN", b"AAN", tab, code, -3, -1)
    assert r["score"] == 2 + 2 - 3 and r["lines"] == (b"AaN", b"*|*", b"AAN")
    assert r["dirH"][1, 1] == 1 and r["dirH"][2, 2] == 2 and r["dirH"][3, 3] == 1
    for kind, (se, sq, sr) in {"ANW": ((0, (0, 0)), (-3 - 3, (0, 3)), (-3 - 2, (2, 0))), "ASW": ((0, (0, 0)),) * 3,
                               "ASG": ((0, (0, 0)), (0, (0, 0)), (-3 - 2, (2, 0)))}.items():
        for (ref, qry), (score, end) in zip(((b"", b""), (b"AAN", b""), (b"", b"AN")), (se, sq, sr)):
            r = dt.align(kind, ref, qry, tab, code, -3, -1)
            assert (r["score"], r["end"]) == (score, end), (kind, ref, qry)
