"""DPX_KEEP_DIRECTIONS on what int16 batches refuse: scores past 32 767 (all three algorithms) and a 70 000-column reference (LSW: the
edge row and the staged reference then live in the batch's allocation instead of LDS).  Checked against the oracle's int32 fills."""
import numpy as np
import pytest

import oracle_py as O
from dpx_gpu_genomics_project_amd.synth import from_strings

pytestmark = pytest.mark.gpu
RANGE = -4


def _near_identical(n, seed, rate=0.02):
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, n).astype(np.uint8) + ord("A")
    q = ref.copy()
    sub = rng.random(n) < rate
    q[sub] = ((q[sub] - ord("A") + 1) % 4 + ord("A")).astype(np.uint8)
    q = np.delete(q, np.nonzero(rng.random(n) < 0.002)[0])
    return ref.tobytes(), q.tobytes()


@pytest.mark.parametrize("algo", ["LNW", "LSW", "ANW"])
def test_scores_beyond_int16(gpu, algo):
    ref, qry = _near_identical(4500, 8)
    sb = from_strings([(ref, qry)])
    code = {"LNW": 0, "LSW": 1, "ANW": 2}[algo]
    w = (8, -4, -6, -1)
    with pytest.raises(gpu.DpxError) as e:  # today's int16 batch: refused, and stays refused
        gpu.Batch(code, sb.sequences, sb.pairs, *w)
    assert e.value.status == RANGE
    with gpu.Batch(code, sb.sequences, sb.pairs, *w, flags=gpu.KEEP_DIRECTIONS) as b:
        b.fill()
        sc, er, ec = b.results()
        lines = b.traceback(0)
    if algo == "LNW":
        r = O.lnw(ref, qry, 8, -4, -6)
        want = O.lnw_traceback(ref, qry, r)
    elif algo == "LSW":
        r = O.lsw(ref, qry, 8, -4, -6)
        want = O.lsw_traceback(ref, qry, r)
        assert (er[0], ec[0]) == (r.end_row, r.end_col)
    else:
        r = O.anw(ref, qry, 8, -4, -6, -1)
        want = O.anw_traceback(ref, qry, r)
    assert r.score > 32767
    assert sc[0] == r.score
    assert lines == want


def test_lsw_reference_of_70000_columns(gpu):
    rng = np.random.default_rng(70)
    ref = (rng.integers(0, 4, 70000).astype(np.uint8) + ord("A"))
    q = ref[41234:41534].copy()
    sub = rng.random(300) < 0.05
    q[sub] = ((q[sub] - ord("A") + 1) % 4 + ord("A")).astype(np.uint8)
    ref, qry = ref.tobytes(), q.tobytes()
    sb = from_strings([(ref, qry)])
    with pytest.raises(gpu.DpxError) as e:
        gpu.Batch(1, sb.sequences, sb.pairs, 3, -1, -2)
    assert e.value.status == RANGE
    with gpu.Batch(1, sb.sequences, sb.pairs, 3, -1, -2, flags=gpu.KEEP_DIRECTIONS) as b:
        assert b.describe()["dir_edges"] == "global"
        b.fill()
        sc, er, ec = b.results()
        lines = b.traceback(0)
        r = O.lsw(ref, qry, 3, -1, -2)
        assert (sc[0], er[0], ec[0]) == (r.score, r.end_row, r.end_col)
        assert lines == O.lsw_traceback(ref, qry, r)
        got = b.directions(0)
        assert np.array_equal(got[:, 41000:42000], r.dir[:, 41000:42000])
        assert np.array_equal(got, r.dir)
