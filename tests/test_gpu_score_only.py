"""DPX_SCORE_ONLY batches of LSW, LNW, ANW and BSW (and, on the lane kernels, ASW and ASG) on the GPU against the CPU oracles the storing
fills are tested with: score, end row and end column of every pair.

STORE = false is another instantiation of every fill kernel, not the storing code minus its stores: k_linear_fill and the affine body
leave the rolling schedule to storing batches (`STORE && S >= 2 && n >= 128`), so a score-only pair of two or more stripes over a
reference of 128 or more columns runs the plain striped loop, which a storing batch never sends that shape to; the lane kernels stage
their references behind kLaneScratch instead of the line stage, run n + skew steps instead of n8 + skew and publish no routing words;
k_banded_fill keeps the key fold only; the planner sizes LDS for no store.  Every case asserts from dpx_batch_describe which kernel=,
rows_per_lane and waves_per_workgroup ran, and waves > 0 exactly for the lane kernels.  _score_only() is the comparator (also of the
score-only cases of tests/test_gpu_layouts.py): results, extension records where the mode writes them, store=0, no pool, and
DPX_ERR_NO_MATRIX from everything that needs stored cells.  The texts, shapes and expectations come from tests/score_only_cases.py
(tests/test_score_only_cases.py asserts their properties on the oracles alone); no expectation comes from another GPU batch."""
import ctypes as C

import pytest

import score_only_cases as S
import zext_ref
from dpx_gpu_genomics_project_amd.capi import DIFF_CS, DIFF_MD, DpxError
from dpx_gpu_genomics_project_amd.synth import from_strings

pytestmark = pytest.mark.gpu

NOT_FILLED, NO_MATRIX = -6, -7
CODE = {"LNW": 0, "LSW": 1, "ANW": 2, "BSW": 3, "ASW": 4, "ASG": 6}
W = S.W
FILL = {"LSW": "k_linear_fill", "LNW": "k_linear_fill", "ANW": "k_affine_fill", "ASW": "k_asw_fill", "ASG": "k_asg_fill", "BSW": "k_banded_fill"}
LANES = {"LSW": "k_linear_lanes", "LNW": "k_linear_lanes", "ANW": "k_affine_lanes", "ASW": "k_asw_lanes", "ASG": "k_asg_lanes"}
KNOBS = ("DPX_R", "DPX_PACKED", "DPX_LANES", "DPX_LANES_PK", "DPX_SPLIT", "DPX_ROW_TAGS", "DPX_RAMP_LINES", "DPX_WPB", "DPX_GROUP", "DPX_TB_WALK")


@pytest.fixture(scope="module")
def oracles(tmp_path_factory):
    return S.build_oracles(tmp_path_factory.mktemp("score_only_oracles"))


@pytest.fixture
def knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


# ------------------------------------------------------------------------------------------------------------------- the comparator

def _status(call, *args):
    try:
        call(*args)
    except DpxError as e:
        return e.status
    return 0


def _score_only(b, want, what=()):
    """the filled score-only batch `b` against `want`, one dict per pair: score, end (row, column) and, where the mode writes extension
    records, rec.  Returns describe()"""
    scores, rows, cols = b.results()
    got = list(zip(scores.tolist(), rows.tolist(), cols.tolist()))
    exp = [(int(r["score"]), int(r["end"][0]), int(r["end"][1])) for r in want]
    bad = [(p, got[p], exp[p]) for p in range(min(len(got), len(exp))) if got[p] != exp[p]]
    assert len(got) == len(exp) == b.num_pairs and not bad, (what, "pair, got, want", bad[:6], len(bad))
    if want and want[0].get("rec") is not None:
        recs = b.extensions()
        for p, r in enumerate(want):
            assert {k: int(recs[k][p]) for k in zext_ref.FIELDS} == r["rec"], (what, p, "extension record")
    d = b.describe()
    assert d["store"] == 0 and d.get("pool_addr", "0x0") == "0x0", d
    calls = [(b.output_begin, 0), (b.cigars_begin, 0), (b.diffs_begin, DIFF_MD | DIFF_CS)]
    if b.num_pairs:
        calls += [(b.matrix, 0), (b.traceback, 0)]
    for call, arg in calls:
        assert _status(call, arg) == NO_MATRIX, (what, call.__name__)
    return d


def _ran(d, algo, kernel, R=None, waves=None, kernel_algo=None):
    assert (d["algo"], d["kernel_algo"], d["kernel"], d["dtype"], d["store"]) == (algo, kernel_algo or algo, kernel, "int32", 0), d
    assert (d["couples"], d["row_tags"]) == (0, 0), d   # (never the packed, split or lanes_pk routes)
    if R is not None:
        assert d["rows_per_lane"] == R, d
    if waves is not None:
        assert d["waves_per_workgroup"] == waves, d
    assert (d["waves"] > 0) == kernel.endswith("_lanes"), d


def _run(gpu, algo, sb, want, kernel, R=None, waves=None, band=0, kernel_algo=None, what=()):
    with gpu.Batch(CODE[algo], sb.sequences, sb.pairs, *W[algo], band=band, flags=gpu.SCORE_ONLY) as b:
        d = b.describe()
        _ran(d, algo, kernel, R, waves, kernel_algo)
        b.fill()
        _score_only(b, want, what)
    return d


# ---- a. the striped loop that only score-only reaches (DPX_LANES=0) ----
@pytest.mark.parametrize("wpb", [1, 4])
@pytest.mark.parametrize("algo,R", S.STRIPED)
def test_striped_loop_of_two_or_more_stripes(gpu, oracles, knobs, algo, R, wpb):
    """two and three stripes (whole and partial last ones) and the single-stripe controls against n = 127, 128, 129, 200 in one batch
    (S.striped_shapes asserts that pairs with S >= 2 and n >= 128 exist): 24 waves of four reference lengths, one per workgroup and four
    per workgroup, where a wave that overruns its LDS slice lands in a neighbour's"""
    knobs.setenv("DPX_LANES", "0")
    knobs.setenv("DPX_R", str(R))
    if wpb != 1:
        knobs.setenv("DPX_WPB", str(wpb))
    sb = S.striped_batch(R)
    want = S.shared(("striped", algo, R), lambda: S.want_of(oracles, algo, sb))
    _run(gpu, algo, sb, want, FILL[algo], R=R, waves=wpb, what=(algo, R, wpb))


# ---- b. LSW's start cell across stripes ----
@pytest.mark.parametrize("R", [2, 8])
def test_lsw_start_cell_across_stripes(gpu, knobs, R):
    """S.tie_want asserts on the oracle's H alone that at least two cells hold the maximum, in different stripes; the GPU reports the
    oracle's cell, the first in row-major order"""
    texts, want = S.shared(("ties", R), lambda: S.tie_want(R))
    sb = from_strings(texts)
    knobs.setenv("DPX_LANES", "0")
    knobs.setenv("DPX_R", str(R))
    for wpb in (1, 4):
        if wpb != 1:
            knobs.setenv("DPX_WPB", str(wpb))
        _run(gpu, "LSW", sb, want, "k_linear_fill", R=R, waves=wpb, what=("ties", R, wpb))
    with gpu.Batch(CODE["LSW"], sb.sequences, sb.pairs, *W["LSW"]) as b:   # in addition: the storing batch of the same inputs
        b.fill()
        s, r, c = b.results()
        assert [(int(s[p]), (int(r[p]), int(c[p]))) for p in range(len(want))] == [(x["score"], x["end"]) for x in want]


# ---- c. the lane kernels (DPX_LANES=1) ----
# (algorithm, the longest query = the kernel's largest 64R, DPX_WPB): the linear kernels run four-wave workgroups unless DPX_WPB=1, the affine
# ones always one-wave workgroups
LANE_CASES = [(algo, top, wpb) for algo in ("LSW", "LNW") for top in (512, 1024) for wpb in (4, 1)] + [(algo, 512, 0) for algo in ("ANW", "ASW", "ASG")]


@pytest.mark.parametrize("algo,top,wpb", LANE_CASES)
def test_lane_kernels(gpu, oracles, knobs, algo, top, wpb):
    """m = 1, 7, 8, 9, 15, 16, 17, 63, 64, 65 and the kernel's largest 64R (512 at 8 rows per lane, the linear kernels' 1024 at 16) against
    n = 1, 7, 8, 9, 90, 257 -- the loop runs n + skew steps where the storing kernel runs n8 + skew -- with empty queries and references in
    the batch"""
    knobs.setenv("DPX_LANES", "1")
    if wpb == 1:
        knobs.setenv("DPX_WPB", "1")
    sb = S.lane_batch(top)
    want = S.shared(("lanes", algo, top), lambda: S.want_of(oracles, algo, sb))
    d = _run(gpu, algo, sb, want, LANES[algo], R=top // 64, waves=wpb or 1, what=(algo, top, wpb))
    assert d["singles"] == 3 and d["lane_pairs"] == sb.num_pairs - 3 and 1 < d["waves"] < d["lane_pairs"], d


@pytest.mark.parametrize("algo", ["LSW", "LNW", "ANW", "ASW", "ASG"])
def test_lane_kernels_ragged40(gpu, oracles, knobs, algo):
    """40 ragged pairs (m 1..256, n 1..260): waves that hold several pairs and empty slots"""
    knobs.setenv("DPX_LANES", "1")
    sb = S.ragged40()
    want = S.shared(("ragged40", algo), lambda: S.want_of(oracles, algo, sb))
    d = _run(gpu, algo, sb, want, LANES[algo], R=8, what=(algo, "ragged40"))
    assert d["lane_pairs"] == 40 and d["singles"] == 0 and 1 < d["waves"] < 40, d


# ---- d. BSW (k_banded_fill) ----
@pytest.mark.parametrize("wpb", [1, 4])
@pytest.mark.parametrize("band", S.BANDS)
def test_bsw(gpu, oracles, knobs, band, wpb):
    """1, 2, 4 and 8 cells per lane, both parities of the band; shapes with and without each of the three phases; S.band_case asserts on
    the oracle that the band changes an answer"""
    knobs.setenv("DPX_PACKED", "0")
    if wpb != 1:
        knobs.setenv("DPX_WPB", str(wpb))
    sb, want = S.band_case(oracles, band)
    cpl = 1 if band <= 64 else 2 if band <= 128 else 4 if band <= 256 else 8
    _run(gpu, "BSW", sb, want, "k_banded_fill", R=cpl, waves=wpb, band=band, what=("BSW", band, wpb))


def test_bsw_covering_band_runs_the_linear_kernel(gpu, oracles, knobs):
    sb = S.batch(77, [(40, 60), (300, 200), (129, 130), (1, 1), (0, 4)])
    band = 300   # >= the longest string: the unbanded recurrence
    want = S.want_of(oracles, "BSW", sb, band)
    assert want == S.want_of(oracles, "LSW", sb)
    knobs.setenv("DPX_LANES", "0")
    d = _run(gpu, "BSW", sb, want, "k_linear_fill", band=band, kernel_algo="LSW", what="covering band")
    assert d["kernel_algo"] == "LSW" and d["store"] == 0


# ---- e. lifecycle ----
@pytest.mark.parametrize("lanes", ["0", "1"])
@pytest.mark.parametrize("algo", ["LSW", "ANW"])
def test_lifecycle(gpu, oracles, knobs, algo, lanes):
    """fill twice and on a caller's non-blocking stream, fill_timed, packed2 input of the same pairs, a batch of zero pairs"""
    knobs.setenv("DPX_LANES", lanes)
    knobs.setenv("DPX_R", "2")
    sb = S.shared("lifecycle", lambda: S.batch(88, [(129, 130), (300, 200), (40, 60), (1, 1), (0, 4), (5, 0), (256, 257), (64, 9)]))
    want = S.shared(("lifecycle", algo), lambda: S.want_of(oracles, algo, sb))
    kernel, R = (LANES[algo], 8) if lanes == "1" else (FILL[algo], 2)
    hip = C.CDLL("libamdhip64.so")   # the runtime the engine itself is linked against
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0 and stream.value   # hipStreamNonBlocking
    try:
        with gpu.Batch(CODE[algo], sb.sequences, sb.pairs, *W[algo], flags=gpu.SCORE_ONLY | gpu.TIME_FILLS) as b:
            d = b.describe()
            _ran(d, algo, kernel, R)
            assert _status(b.results) == NOT_FILLED
            b.fill(stream.value)   # no synchronisation between create and this fill
            _score_only(b, want, (algo, lanes, "caller's stream"))
            for k in range(2):
                b.fill()
                _score_only(b, want, (algo, lanes, "fill", k))
            assert b.fill_timed(3) > 0
            _score_only(b, want, (algo, lanes, "fill_timed"))
    finally:
        assert hip.hipStreamDestroy(stream) == 0
    packed, alphabet = gpu.pack2(sb.sequences, sb.pairs)
    with gpu.Batch(CODE[algo], None, sb.pairs, *W[algo], flags=gpu.SCORE_ONLY, packed2=(packed, alphabet, sb.sequences.size)) as b:
        d = b.describe()
        _ran(d, algo, kernel, R)
        assert d["seq_input"] == "packed2", d
        b.fill()
        _score_only(b, want, (algo, lanes, "packed2"))
    with gpu.Batch(CODE[algo], sb.sequences, sb.pairs, *W[algo], flags=gpu.SCORE_ONLY, num_pairs=0) as b:
        d = b.describe()
        assert (d["algo"], d["store"], d["singles"], d["waves"]) == (algo, 0, 0, 0), d
        b.fill()
        _score_only(b, [], (algo, lanes, "zero pairs"))
