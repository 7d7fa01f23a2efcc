"""ANW / ASW / ASG direction batches under dpx_batch_set_direction_table (k_dirtab_fill) on the GPU, bit-exact against the CPU oracle
tests/dirtab_oracle.c (int64 cells): scores, end cells, exported enum planes, traceback lines, the text block and the CIGAR records.
Every case asserts from dpx_batch_describe which kernel=, rows_per_lane, subst=, dir_edges and waves_per_workgroup ran.  The tables are
random and asymmetric (a transposed lookup fails) unless a case says otherwise."""
import ctypes as C

import numpy as np
import pytest

import cigar_ref
import dirtab_ref
import poison
import subst_ref
from dpx_gpu_genomics_project_amd.synth import from_strings

pytestmark = pytest.mark.gpu

INVALID, RANGE, NOT_FILLED, NO_MATRIX, UNSUPPORTED = -1, -4, -6, -7, -8
ALGO = {"ANW": 2, "ASW": 4, "ASG": 6}
KERNEL = {"ANW": "k_affine_dir", "ASW": "k_asw_dir", "ASG": "k_asg_dir"}
KINDS = sorted(ALGO)
GAPS = (-4, -1)
MM = (1, -1)  # params.match / params.mismatch: ignored under a table
ALPHABETS = (1, 2, 5, 24, 32)
LETTERS = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmn", np.uint8)  # 40 byte values: byte equality is rarer than code equality
KNOBS = ("DPX_R", "DPX_WPB", "DPX_POOL", "DPX_POOL_GUARD", "DPX_GROUP")
LDS_MAX, IMAGE = 160 * 1024, 1280


@pytest.fixture(scope="module")
def dt(tmp_path_factory):
    return dirtab_ref.build(tmp_path_factory.mktemp("dirtab_gpu"))


@pytest.fixture
def knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _status(gpu, call, *args):
    try:
        call(*args)
    except gpu.DpxError as e:
        return e.status
    return 0


def _related(rng, n, m, letters=LETTERS, subs=0.15):
    """a reference of n letters and a query of m: the reference (cyclically) with substitutions, one deletion and one insertion"""
    if n == 0 or m == 0:
        return letters[rng.integers(0, len(letters), n)].tobytes(), letters[rng.integers(0, len(letters), m)].tobytes()
    ref = rng.integers(0, len(letters), n)
    q = np.resize(ref, m).copy()
    hit = rng.random(m) < subs
    q[hit] = rng.integers(0, len(letters), int(hit.sum()))
    if m > 30:
        q = np.resize(np.concatenate([q[:10], q[13:m // 2], rng.integers(0, len(letters), 2), q[m // 2:]]), m)
    return letters[ref].tobytes(), letters[q].tobytes()


def _dir_per_wave(n):
    """main_lds (dpx_plan.cpp): two int32 edge rows of n + 2 and the staged reference of n + 192 bytes, each rounded up to 16"""
    return 2 * (-(-((n + 2) * 4) // 16) * 16) + -(-(n + 192) // 16) * 16


def _ran(d, kind, R, alphabet, edges="lds", waves=None):
    assert (d["algo"], d["kernel_algo"], d["kernel"], d["dtype"], d["matrix"]) == (kind, kind, KERNEL[kind], "int32", "dir4"), d
    assert d["rows_per_lane"] == R and d.get("subst") == (alphabet or None) and d["dir_edges"] == edges, d
    if waves is not None:
        assert d["waves_per_workgroup"] == waves, d


def _observe(gpu, b, picks="all", number=5):
    """everything a filled direction batch reports"""
    scores, rows, cols = b.results()
    out = {"scores": scores.tolist(), "ends": list(zip(rows.tolist(), cols.tolist())),
           "lines": [tuple(x.encode("latin-1") for x in b.traceback(p)) for p in range(b.num_pairs)]}
    b.output_begin(number)
    out["text"] = b.output_end()[0]
    b.cigars_begin(gpu.CIGAR_EXTENDED)
    recs, ops = b.cigars_end()
    out["recs"], out["ops"] = recs, [int(x) for x in ops]
    picks = range(b.num_pairs) if picks == "all" else picks
    out["dirs"] = {p: [b.directions(p, which) for which in (gpu.MAT_H, gpu.MAT_I, gpu.MAT_D)] for p in picks}
    return out


def _want(dt, kind, sb, table, code, gaps=GAPS):
    return [dt.align(kind, sb.ref(p), sb.qry(p), table, code, *gaps) for p in range(sb.num_pairs)]


def _against(got, want, tag, number=5):
    for p, r in enumerate(want):
        assert (got["scores"][p], got["ends"][p]) == (r["score"], r["end"]), (tag, p)
        assert got["lines"][p] == r["lines"], (tag, p)
    for p, planes in got["dirs"].items():
        for key, have in zip(("dirH", "dirI", "dirD"), planes):
            assert np.array_equal(have, want[p][key]), (tag, p, key, np.argwhere(have != want[p][key])[:4])
    assert got["text"] == b"".join(b"%d | %d\n" % (number + p, r["score"]) + b"".join(x + b"\n" for x in r["lines"]) for p, r in enumerate(want)), tag
    records, flat = cigar_ref.batch([r["lines"] for r in want], [r["end"][0] for r in want], [r["end"][1] for r in want])
    assert got["ops"] == flat, tag
    for p, rec in enumerate(records):
        for field, value in rec.items():
            assert int(got["recs"][field][p]) == value, (tag, p, field)


def _same(a, b, tag):
    for key in ("scores", "ends", "lines", "text", "ops"):
        assert a[key] == b[key], (tag, key)
    assert a["recs"].tobytes() == b["recs"].tobytes(), tag
    assert sorted(a["dirs"]) == sorted(b["dirs"])
    for p in a["dirs"]:
        assert all(np.array_equal(x, y) for x, y in zip(a["dirs"][p], b["dirs"][p])), (tag, p)


def _check(gpu, dt, kind, sb, table, code, R, gaps=GAPS, mm=MM, edges="lds", waves=None, picks="all", fill=None, want=None, **kw):
    """one direction batch under the table against the oracle; returns (describe, observations, expectations)"""
    want = _want(dt, kind, sb, table, code, gaps) if want is None else want
    with gpu.Batch(ALGO[kind], sb.sequences, sb.pairs, *mm, *gaps, flags=gpu.KEEP_DIRECTIONS, **kw) as b:
        _ran(b.describe(), kind, R, 0, edges)
        b.set_direction_table(table, code)
        d = b.describe()
        _ran(d, kind, R, np.asarray(table).shape[0], edges, waves)
        (fill or (lambda batch: batch.fill()))(b)
        assert _status(gpu, b.matrix, 0) == NO_MATRIX
        got = _observe(gpu, b, picks)
    _against(got, want, (kind, R, np.asarray(table).shape[0]))
    return d, got, want


# ---- 1. rows per lane and stripes ----
MS = (1, 2, 63, 64, 65, 127, 128, 129, 256, 257, 512, 513, 600)
NS = (1, 2, 63, 64, 65, 130, 300)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", MS)
def test_rows_per_lane_and_stripes(gpu, dt, knobs, kind, m):
    """one batch per query length, every reference length in it; R = 2 / 4 / 8 by plan, two stripes at R = 8 from 513 rows on; the
    alphabets 1, 2, 5, 24, 32 go round the query lengths, shifted per algorithm so that each meets each R"""
    rng = np.random.default_rng(1000 * ALGO[kind] + m)
    alphabet = ALPHABETS[(MS.index(m) + KINDS.index(kind)) % len(ALPHABETS)]
    table, code = dirtab_ref.random_table(rng, alphabet)
    sb = from_strings([_related(rng, n, m) for n in NS])
    R = 2 if m <= 128 else 4 if m <= 256 else 8
    _check(gpu, dt, kind, sb, table, code, R, picks="all" if m <= 129 else (0, 3, 6))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", (129, 257, 300))
def test_stripes_at_two_rows_per_lane(gpu, dt, knobs, kind, m):
    """DPX_R=2: stripes of 128 rows -- two, three with one row in the last, three with a partial last stripe"""
    knobs.setenv("DPX_R", "2")
    rng = np.random.default_rng(2000 * ALGO[kind] + m)
    table, code = dirtab_ref.random_table(rng, ALPHABETS[(m + KINDS.index(kind)) % len(ALPHABETS)])
    sb = from_strings([_related(rng, n, m) for n in (1, 64, 65, 300)])
    _check(gpu, dt, kind, sb, table, code, 2)


@pytest.mark.parametrize("kind", KINDS)
def test_ragged_batch(gpu, dt, knobs, kind):
    """40 pairs of every size up to 300 x 300, empty sequences among them: the launch order (longest first) and lanes without rows"""
    rng = np.random.default_rng(3000 + ALGO[kind])
    sizes = [(int(rng.integers(0, 301)), int(rng.integers(0, 301))) for _ in range(36)] + [(0, 0), (0, 40), (40, 0), (300, 300)]
    sb = from_strings([_related(rng, n, m) for n, m in sizes])
    table, code = dirtab_ref.random_table(rng, 24)
    d, _, _ = _check(gpu, dt, kind, sb, table, code, 8, picks=range(0, 40, 3))
    assert d["singles"] == 40, d


# ---- 2. the table that scores as byte equality does ----
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m,R", [(100, 2), (200, 4), (400, 8)])
def test_identity_table_equals_the_plain_batch(gpu, dt, knobs, kind, m, R):
    rng = np.random.default_rng(4000 + ALGO[kind] + m)
    letters = LETTERS[:20]
    sb = from_strings([_related(rng, n, m, letters) for n in (90, 150, 333)] + [_related(rng, 50, m // 2, letters)])
    table, code = subst_ref.identity_table(3, -1, letters.tobytes())
    with gpu.Batch(ALGO[kind], sb.sequences, sb.pairs, 3, -1, *GAPS, flags=gpu.KEEP_DIRECTIONS) as b:
        _ran(b.describe(), kind, R, 0)
        b.fill()
        plain = _observe(gpu, b)
    _, got, _ = _check(gpu, dt, kind, sb, table, code, R, mm=(1, -1))
    _same(got, plain, (kind, m))


# ---- 3. where the edge rows live ----
@pytest.mark.parametrize("kind", KINDS)
def test_four_waves_become_one_between_the_two_thresholds(gpu, dt, knobs, kind):
    """a reference whose four waves' edge rows and stage fit a workgroup's LDS without the table image and not with it"""
    n = 4480
    assert 4 * _dir_per_wave(n) <= LDS_MAX < 4 * (_dir_per_wave(n) + IMAGE)
    knobs.setenv("DPX_WPB", "4")
    rng = np.random.default_rng(5000 + ALGO[kind])
    sb = from_strings([_related(rng, n, 70), _related(rng, n - 7, 69), _related(rng, 100, 70)])
    table, code = dirtab_ref.random_table(rng, 24)
    with gpu.Batch(ALGO[kind], sb.sequences, sb.pairs, *MM, *GAPS, flags=gpu.KEEP_DIRECTIONS) as b:
        assert b.describe()["waves_per_workgroup"] == 4
    _check(gpu, dt, kind, sb, table, code, 2, waves=1, picks=(2,))
    short = from_strings([_related(rng, 4300, 70), _related(rng, 100, 70)])  # ... and below the lower threshold the four waves stay
    assert 4 * (_dir_per_wave(4300) + IMAGE) <= LDS_MAX
    _check(gpu, dt, kind, short, table, code, 2, waves=4, picks=(1,))


@pytest.mark.parametrize("kind", KINDS)
def test_global_edge_rows_two_stripes(gpu, dt, knobs, kind):
    """a reference just past the 64 KiB of one wave's LDS slice: edge rows and stage in the scratch, the table image alone in LDS"""
    knobs.setenv("DPX_R", "2")
    n = next(x for x in range(7000, 8000) if _dir_per_wave(x) > 64 * 1024)
    assert 7200 < n < 7300
    rng = np.random.default_rng(6000 + ALGO[kind])
    sb = from_strings([_related(rng, n, 130), _related(rng, 200, 129)])
    table, code = dirtab_ref.random_table(rng, 5)
    d, _, _ = _check(gpu, dt, kind, sb, table, code, 2, edges="global", waves=1, picks=(1,))
    assert d["dir_scratch_bytes"] > 0, d


# ---- 4. ties and zeros ----
@pytest.mark.parametrize("kind", KINDS)
def test_ties_and_zeros(gpu, dt, knobs, kind):
    """two letters, m and n in 0..13, under the four fuzz tables: ASW's first strict maximum and H == 0 stops, ASG's column-0 tie, every
    tie of the tie order; empty sequences included"""
    code = subst_ref.fuzz_code()
    texts = subst_ref.fuzz_pairs(1, False) + subst_ref.fuzz_pairs(2, False)
    assert any(not r for r, _ in texts) and any(not q for _, q in texts)
    sb = from_strings(texts)
    zero_scores = 0
    for table in subst_ref.FUZZ_TABLES:
        _, got, _ = _check(gpu, dt, kind, sb, np.array(table, np.int8), code, 2, gaps=subst_ref.FUZZ_GAPS)
        zero_scores += sum(s == 0 for s in got["scores"])
    assert zero_scores > 0


# ---- 5. what the table means ----
def test_negative_n_folded_case_and_scores_past_int16(gpu, dt, knobs):
    code = gpu.code_table(b"ACGTN")
    table = np.full((5, 5), -3, np.int8)
    np.fill_diagonal(table, 2)
    table[4, :] = table[:, 4] = -1
    sb = from_strings([(b"ACGTNNNNACGT", b"ACGTNNNNACGT"), (b"ACGTACGTAC", b"acgtACGTac"), (b"NNNN", b"NNNN")])
    for kind in KINDS:
        _, got, want = _check(gpu, dt, kind, sb, table, code, 2)
        assert got["lines"][0][1] == b"*" * 12 and got["scores"][0] == 8 * 2 - 4  # N against N scores -1 and still prints '*' (equal bytes)
        assert got["scores"][1] == 20 and got["lines"][1][1] == b"||||****||"   # folded case scores as a match and prints by byte equality
        assert got["scores"][2] == (0 if kind == "ASW" else -4), got["scores"]
    rng = np.random.default_rng(55)
    big = rng.integers(100, 128, (24, 24)).astype(np.int8)
    same = LETTERS[rng.integers(0, 24, 700)].tobytes()
    long = from_strings([(same, same), _related(rng, 690, 700, LETTERS[:24], subs=0.05)])
    for kind in KINDS:
        _, got, _ = _check(gpu, dt, kind, long, big, gpu.code_table(LETTERS[:24].tobytes(), fold_case=False), 8, picks=())
        assert min(got["scores"]) > 32767 and got["scores"][0] >= 700 * 100, got["scores"]


# ---- 6. lifecycle and refusals ----
def test_changes_between_fills(gpu, dt, knobs):
    rng = np.random.default_rng(60)
    sb = from_strings([_related(rng, 150, 140), _related(rng, 90, 100), _related(rng, 30, 200)])
    t1, code = dirtab_ref.random_table(rng, 5)
    t2 = t1.T.copy()
    for kind in KINDS:
        with gpu.Batch(ALGO[kind], sb.sequences, sb.pairs, 3, -1, *GAPS, flags=gpu.KEEP_DIRECTIONS) as b:
            calls = (b.results, lambda: b.traceback(0), lambda: b.directions(0, 0), lambda: b.output_begin(0), b.cigars_begin)
            b.fill()
            plain = _observe(gpu, b)
            b.set_direction_table(None)  # nothing was set: nothing changes
            assert _status(gpu, b.results) == 0
            for table in (t1, t2):
                b.set_direction_table(table, code)
                for call in calls:
                    assert _status(gpu, call) == NOT_FILLED, kind
                _ran(b.describe(), kind, 4, 5)
                b.fill()
                _against(_observe(gpu, b), _want(dt, kind, sb, table, code), (kind, "step"))
                b.set_direction_table(table, code)  # the same table again keeps the fill
                assert _status(gpu, b.results) == 0
                # the three old setters still refuse a direction batch that has a table
                before = b.describe()
                assert _status(gpu, b.set_substitution, t1, code) == UNSUPPORTED and _status(gpu, b.set_extension_table, 7, 7, t1, code) == UNSUPPORTED
                assert _status(gpu, b.set_direction_scoring, -1, -1, t1, code) == UNSUPPORTED and _status(gpu, b.set_extension, 7, 7) == UNSUPPORTED
                assert b.describe() == before and _status(gpu, b.results) == 0
            b.set_direction_table(None)
            _ran(b.describe(), kind, 4, 0)
            assert _status(gpu, b.results) == NOT_FILLED
            b.fill()
            _same(_observe(gpu, b), plain, (kind, "cleared"))


def test_invalid_arguments_and_unsupported_batches(gpu, knobs):
    rng = np.random.default_rng(61)
    sb = from_strings([_related(rng, 90, 80, LETTERS[:4]), _related(rng, 70, 75, LETTERS[:4])])
    table, code = dirtab_ref.random_table(rng, 5)
    t8 = np.ascontiguousarray(table, np.int8)
    lib = gpu.load()
    raw = lambda b, s, a, c: lib.dpx_batch_set_direction_table(b._h if b is not None else None, s, a, c)
    assert raw(None, t8.ctypes.data, 5, code.ctypes.data) == INVALID and raw(None, None, 0, None) == INVALID
    with gpu.Batch(ALGO["ASW"], sb.sequences, sb.pairs, *MM, *GAPS, flags=gpu.KEEP_DIRECTIONS) as b:
        b.set_direction_table(table, code)
        before = b.describe()
        bad = code.copy()
        bad[7] = 5
        for args in ((t8.ctypes.data, 0, code.ctypes.data), (t8.ctypes.data, 33, code.ctypes.data), (t8.ctypes.data, -1, code.ctypes.data),
                     (t8.ctypes.data, 5, None), (t8.ctypes.data, 5, bad.ctypes.data)):
            assert raw(b, *args) == INVALID, args
            assert b.describe() == before
        assert raw(b, None, 77, bad.ctypes.data) == 0 and "subst" not in b.describe()  # scores == NULL: the other arguments are ignored
    G = gpu
    others = [(a, 0, f) for a in (2, 4, 6) for f in (G.KEEP_MATRICES, G.SCORE_ONLY)]           # matrix and score-only batches of the three
    others += [(0, 0, G.KEEP_DIRECTIONS), (1, 0, G.KEEP_DIRECTIONS)]                           # LNW / LSW direction batches
    others += [(a, 20, f) for a in (3, 5, 7, 10) for f in (G.KEEP_MATRICES, G.SCORE_ONLY)]     # every banded algorithm ...
    others += [(7, 20, G.KEEP_BAND_DIRECTIONS), (10, 20, G.KEEP_BAND_DIRECTIONS), (7, 20, G.KEEP_BAND_DIRECTIONS | G.TWO_PIECE_GAPS),
               (3, 20, G.KEEP_LOCAL_BAND_DIRECTIONS), (5, 20, G.KEEP_LOCAL_BAND_DIRECTIONS)]     # ... in every storage mode
    covering = {(7, 200, G.KEEP_BAND_DIRECTIONS): "k_affine_dir", (3, 200, G.KEEP_LOCAL_BAND_DIRECTIONS): "k_linear_dir",
                (5, 200, G.KEEP_LOCAL_BAND_DIRECTIONS): "k_asw_dir"}                             # covering bands that run the direction kernels
    for algo, band, flags in others + list(covering):
        with gpu.Batch(algo, sb.sequences, sb.pairs, *MM, *GAPS, band=band, flags=flags) as o:
            before = o.describe()
            if (algo, band, flags) in covering:
                assert before["kernel"] == covering[algo, band, flags] and before["matrix"] == "dir4", before
            assert _status(gpu, o.set_direction_table, table, code) == UNSUPPORTED, (algo, band, flags)
            assert o.describe() == before
            o.set_direction_table(None)  # the clear is legal on every batch, and changes nothing where nothing was set
            assert o.describe() == before


def test_range_refusal_keeps_the_previous_table(gpu, dt, knobs):
    """fits_dir for ASW: max(match, 0) * min(m, n) + (max(o, 0) + max(e, 0)) * (m + n) + max(o, 0) + max(e, 0) * max(m, n) <= 2^28.
    With m = n = L, e < 0 and the largest o that passes at match = 1, an entry of 127 in its place does not pass."""
    L = 2000
    o = ((1 << 28) - L) // (2 * L + 1)
    assert 1 * L + o * (2 * L + 1) <= (1 << 28) < 127 * L + o * (2 * L + 1) and o <= (1 << 20)
    rng = np.random.default_rng(62)
    sb = from_strings([_related(rng, L, L, LETTERS[:5])])
    code = gpu.code_table(LETTERS[:5].tobytes(), fold_case=False)
    small = np.where(np.eye(5, dtype=bool), 1, -2).astype(np.int8)
    small[0, 1] = -1
    with gpu.Batch(ALGO["ASW"], sb.sequences, sb.pairs, 1, -1, o, -1, flags=gpu.KEEP_DIRECTIONS) as b:
        b.set_direction_table(small, code)
        b.fill()
        before = b.describe()
        big = small.copy()
        big[3, 3] = 127
        assert _status(gpu, b.set_direction_table, big, code) == RANGE
        assert b.describe() == before and before["subst"] == 5
        scores, rows, cols = b.results()  # ... and the earlier fill stays valid
        want = dt.align("ASW", sb.ref(0), sb.qry(0), small, code, o, -1)
        assert (int(scores[0]), (int(rows[0]), int(cols[0]))) == (want["score"], want["end"])
        b.fill()  # the previous table is still the one in force
        assert int(b.results()[0][0]) == want["score"]
    # (o is the limit: one more and the creation's own check refuses the batch at match = 1)
    assert _status(gpu, lambda: gpu.Batch(ALGO["ASW"], sb.sequences, sb.pairs, 1, -1, o + 1, -1, flags=gpu.KEEP_DIRECTIONS)) == RANGE


# ---- 7. plumbing ----
def test_plumbing(gpu, dt, knobs):
    """packed2 input, a caller's stream with repeated fills, DPX_TIME_FILLS, dpx_batch_fill_timed and dpx_batch_create_on"""
    rng = np.random.default_rng(70)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    sb = from_strings([_related(rng, int(rng.integers(20, 300)), int(rng.integers(20, 300)), acgt) for _ in range(29)] + [_related(rng, 300, 280, acgt)])
    table, code = dirtab_ref.random_table(rng, 5)
    hip = C.CDLL("libamdhip64.so")
    handle = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(handle), 1) == 0 and handle.value   # hipStreamNonBlocking
    pk, al = gpu.pack2(sb.sequences, sb.pairs)

    def three_fills_on_the_stream(b):
        for _ in range(3):
            b.fill(handle.value)

    def timed(b):
        usec = C.c_double(0.0)
        assert gpu.load().dpx_batch_fill_timed(b._h, 2, C.byref(usec)) == 0 and usec.value > 0

    for kind in KINDS:
        want = _want(dt, kind, sb, table, code)
        for kw, fill in (({}, three_fills_on_the_stream), ({"packed2": (pk, al, sb.sequences.size)}, None), ({"device": 0}, timed)):
            d, _, _ = _check(gpu, dt, kind, sb, table, code, 8, want=want, picks=range(0, 30, 7), fill=fill, **kw)
            assert d["seq_input"] == ("packed2" if "packed2" in kw else "bytes")
        with gpu.Batch(ALGO[kind], sb.sequences, sb.pairs, *MM, *GAPS, flags=gpu.KEEP_DIRECTIONS | gpu.TIME_FILLS) as b:
            b.set_direction_table(table, code)
            b.fill(handle.value)
            usec = C.c_double(0.0)
            assert gpu.load().dpx_batch_last_fill_usec(b._h, C.byref(usec)) == 0 and usec.value > 0
            _against(_observe(gpu, b, ()), want, (kind, "timed fills"))
    assert hip.hipStreamDestroy(handle) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_stale_pool_bytes_reach_nothing(gpu, dt, knobs, kind):
    """the pool (codes and, with global edge rows, the scratch behind them) overwritten between fills: nothing reported depends on it"""
    knobs.setenv("DPX_R", "2")
    n = next(x for x in range(7000, 8000) if _dir_per_wave(x) > 64 * 1024)
    rng = np.random.default_rng(80 + ALGO[kind])
    table, code = dirtab_ref.random_table(rng, 5)
    for sb, edges in ((from_strings([_related(rng, 100, 140), _related(rng, 33, 5), _related(rng, 0, 9)]), "lds"),
                      (from_strings([_related(rng, n, 130), _related(rng, 50, 20)]), "global")):
        want = _want(dt, kind, sb, table, code)
        seen = []
        with gpu.Batch(ALGO[kind], sb.sequences, sb.pairs, *MM, *GAPS, flags=gpu.KEEP_DIRECTIONS) as b:
            b.set_direction_table(table, code)
            _ran(b.describe(), kind, 2, 5, edges)
            for byte in (0xFF, 0x5A):
                poison.poison(b, byte)
                b.fill()
                got = _observe(gpu, b, picks=(sb.num_pairs - 1, sb.num_pairs - 2))
                _against(got, want, (kind, "poison", byte))
                seen.append(got)
        _same(seen[0], seen[1], (kind, edges))
