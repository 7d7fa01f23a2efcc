"""Band-direction batches under dpx_batch_set_direction_scoring (k_bdx_fill) on the GPU, bit-exact against the CPU oracles: records,
chosen score and end cell, traceback lines, text, and the exported direction planes masked behind lastDiag.  Expected values come from
tests/zsub_oracle.c (int64 cells: no int16 limit) through bdx_ref.expect, for the 33 000-base pair from tests/bdx_oracle.c, and where a
matrix batch admits the same input also from that batch under the corresponding old setter.  Every case asserts from
dpx_batch_describe that k_bdx_fill ran.  Modes without a table score by params.match / params.mismatch; the oracle is then given the
table that scores as byte equality does."""
import ctypes as C

import numpy as np
import pytest

import bdx_ref
import poison
import subst_ref
import zsub_ref
from bdx_ref import BANW, BAXT, MODES
from dpx_gpu_genomics_project_amd.synth import from_strings

pytestmark = pytest.mark.gpu

INVALID, RANGE, NOT_FILLED, NO_MATRIX, UNSUPPORTED = -1, -4, -6, -7, -8
TABLE, CODE = zsub_ref.acgtn_table()
GAPS = zsub_ref.GAPS
MM = (2, -3)  # params.match / params.mismatch of the modes without a table; ignored under one
ACGT = np.frombuffer(b"ACGT", np.uint8)
NAME = {BANW: "BANW", BAXT: "BAXT"}


@pytest.fixture(scope="module")
def zs(tmp_path_factory):
    return zsub_ref.build(tmp_path_factory.mktemp("bdx_gpu"))


@pytest.fixture(scope="module")
def bo(tmp_path_factory):
    return bdx_ref.build(tmp_path_factory.mktemp("bdx_gpu_band"))


def _status(gpu, call, *args):
    try:
        call(*args)
    except gpu.DpxError as e:
        return e.status
    return 0


def _ran_bdx(d, algo, band, z, e, alphabet):
    assert d["algo"] == NAME[algo] and d["kernel_algo"] == NAME[algo] and d["kernel"] == "k_bdx_fill", d
    assert d["traceback"] == "k_bdir_traceback" and d["matrix"] == "banddir4" and d["dtype"] == "int32", d
    assert d["rows_per_lane"] == bdx_ref.cpl(band), d
    assert (d.get("zdrop"), d.get("end_bonus")) == ((z, e) if (z >= 0 or e >= 0) else (None, None)), d
    assert d.get("subst") == (alphabet or None), d


def _records(b):
    return [{k: int(r[k]) for k in zsub_ref.FIELDS} for r in b.extensions()]


def _observe(gpu, b, picks="all", scan=True, cigars=True):
    """everything a filled band-direction batch reports"""
    scores, rows, cols = b.results()
    out = {"scores": scores.tolist(), "ends": list(zip(rows.tolist(), cols.tolist())),
           "lines": [tuple(x.encode("latin-1") for x in b.traceback(p)) for p in range(b.num_pairs)]}
    out["recs"] = _records(b) if scan else _status(gpu, b.extensions)
    b.output_begin(5)
    out["text"] = b.output_end()[0]
    if cigars:
        b.cigars_begin(gpu.CIGAR_EXTENDED)
        recs, ops = b.cigars_end()
        out["cigar"] = (recs.tobytes(), ops.tolist())
    picks = range(b.num_pairs) if picks == "all" else picks
    out["dirs"] = {p: [b.directions(p, which) for which in (gpu.MAT_H, gpu.MAT_I, gpu.MAT_D)] for p in picks}
    return out


def _against(got, want, tag, scan):
    for p, r in enumerate(want):
        if scan:
            assert got["recs"][p] == r["rec"], (tag, p, got["recs"][p], r["rec"])
        assert (got["scores"][p], got["ends"][p]) == (r["score"], r["end"]), (tag, p)
        assert got["lines"][p] == r["lines"], (tag, p)
    if not scan:
        assert got["recs"] == UNSUPPORTED, tag  # a fill that did not run the scan has no records
    for p, planes in got["dirs"].items():
        for key, have, exp in zip("HID", planes, want[p]["dirs"]):
            assert np.array_equal(have, exp), (tag, p, key, want[p]["rec"], np.argwhere(have != exp)[:4])
    assert got["text"] == b"".join(b"%d | %d\n" % (5 + p, r["score"]) + b"".join(x + b"\n" for x in r["lines"]) for p, r in enumerate(want)), tag


def _oracle_table(table, code, mm, used):
    return (np.asarray(table, np.int8), code) if table is not None else bdx_ref.byte_table(*mm, used)


def _want(zs, sb, algo, band, z, e, table, code, gaps, mm=MM, used=b"ACGTN"):
    t, c = _oracle_table(table, code, mm, used)
    return [bdx_ref.expect(zs, sb.ref(p), sb.qry(p), t, c, *gaps, band, algo == BAXT, z, e) for p in range(sb.num_pairs)]


def _check(gpu, zs, sb, algo, band, z=-1, e=-1, table=None, code=None, gaps=GAPS, mm=MM, used=b"ACGTN", want=None, picks="all", fill=None, **kw):
    """one band-direction batch in one mode against the oracle; returns (describe, observations, expectations)"""
    want = _want(zs, sb, algo, band, z, e, table, code, gaps, mm, used) if want is None else want
    scan = z >= 0 or e >= 0
    with gpu.Batch(algo, sb.sequences, sb.pairs, *mm, *gaps, band=band, flags=gpu.KEEP_BAND_DIRECTIONS, **kw) as b:
        assert b.describe()["kernel"] == "k_bdir_fill"
        b.set_direction_scoring(z, e, table, code)
        d = b.describe()
        _ran_bdx(d, algo, band, z, e, 0 if table is None else np.asarray(table).shape[0])
        (fill or (lambda batch: batch.fill()))(b)
        assert _status(gpu, b.matrix, 0) == NO_MATRIX
        got = _observe(gpu, b, picks, scan)
    _against(got, want, (NAME[algo], band, z, e, table is not None), scan)
    return d, got, want


def _matrix_batch(gpu, sb, algo, band, z, e, table, code, gaps=GAPS, mm=MM, **kw):
    """the same input as a matrix batch under the corresponding old setter"""
    with gpu.Batch(algo, sb.sequences, sb.pairs, *mm, *gaps, band=band, **kw) as mb:
        scan = z >= 0 or e >= 0
        if table is not None and scan:
            mb.set_extension_table(z, e, table, code)
        elif table is not None:
            mb.set_substitution(table, code)
        else:
            mb.set_extension(z, e)
        mb.fill()
        scores, rows, cols = mb.results()
        out = {"scores": scores.tolist(), "ends": list(zip(rows.tolist(), cols.tolist())),
               "lines": [tuple(x.encode("latin-1") for x in mb.traceback(p)) for p in range(mb.num_pairs)],
               "recs": _records(mb) if scan else None}
        mb.output_begin(5)
        out["text"] = mb.output_end()[0]
        mb.cigars_begin(gpu.CIGAR_EXTENDED)
        recs, ops = mb.cigars_end()
        out["cigar"] = (recs.tobytes(), ops.tolist())
    return out


def _same_as_matrix(got, other, tag):
    for key in ("scores", "ends", "lines", "text", "cigar"):
        assert got[key] == other[key], (tag, key)
    if other["recs"] is not None:
        assert got["recs"] == other["recs"], tag


def _mode_args(mode, z, e, table, code):
    _, algo, with_table, drop, bonus = mode
    return algo, (z if drop else -1), (e if bonus else -1), (table if with_table else None), (code if with_table else None)


# ---- 1. the fuzz set, all six modes ----
@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_fuzz(gpu, zs, mode):
    code = subst_ref.fuzz_code()
    batches = 0
    for band, texts in zsub_ref.fuzz_texts().items():
        if mode[1] == BANW:
            texts = [t for t in texts if abs(len(t[0]) - len(t[1])) < band]
        sb = from_strings(texts)
        for k, table in enumerate(zsub_ref.FUZZ_TABLES):
            symmetric = table[0][1] == table[1][0]
            if not mode[2] and not symmetric:
                continue  # (not a match / mismatch pair)
            for z in (zsub_ref.FUZZ_Z if mode[3] else (-1,)):
                algo, zz, ee, tab, cod = _mode_args(mode, z, zsub_ref.FUZZ_E, np.array(table, np.int8), code)
                mm = (table[0][0], table[0][1]) if not mode[2] else (1, -1)
                _, got, _ = _check(gpu, zs, sb, algo, band, zz, ee, tab, cod, gaps=zsub_ref.FUZZ_GAPS, mm=mm, used=b"AB")
                if k == 3 or (not mode[2] and k == 2):  # once per band and Z: the matrix batch says the same
                    _same_as_matrix(got, _matrix_batch(gpu, sb, algo, band, zz, ee, tab, cod, gaps=zsub_ref.FUZZ_GAPS, mm=mm), (mode[0], band, z))
                batches += 1
    assert batches >= 10


# ---- 2. the drop sweep ----
def _extra_pairs(rng, band):
    """a pair that never drops (the query is a prefix of the reference: the anti-diagonal after a match falls by 6, no more than Z = 7
    plus the gap's penalty allows), and one that the end bonus flips (the query's last base mismatches: row m's best lies 3 below the
    maximum, within E = 5)"""
    L = bdx_ref.SWEEP_BANDS[band] + 3
    p = ACGT[rng.integers(0, 4, L)].tobytes()
    last = b"A" if p[-1:] != b"A" else b"C"
    return [(p + b"ACGT" * 6, p), (p, p[:-1] + last)]


@pytest.mark.parametrize("with_table", [True, False], ids=["table", "bytes"])
@pytest.mark.parametrize("band", sorted(bdx_ref.SWEEP_BANDS))
def test_drop_sweep(gpu, zs, band, with_table):
    cases = bdx_ref.sweep_cases(band)
    extra = _extra_pairs(np.random.default_rng(band), band)
    # bands of 100 and up: the pairs with long tails, whose drops lie in the fill's interior phase (the sweep's own lie in its tail
    # phase from a band of about 114 on); tests/test_bdx_oracle.py holds every C to an interior drop on either step of the loop body
    inner = bdx_ref.interior_cases(band) if band in bdx_ref.INTERIOR_BANDS else []
    sb = from_strings([(r, q) for _, r, q in cases] + extra + [(r, q) for _, r, q, _ in inner])
    table, code = (TABLE, CODE) if with_table else (None, None)
    gd = 32 // bdx_ref.cpl(band)
    seen = set()
    for z in bdx_ref.SWEEP_Z if with_table else (7,):
        d, got, want = _check(gpu, zs, sb, BAXT, band, z, bdx_ref.SWEEP_E, table, code)  # (the planes of every pair: behind a late drop
        # the export alone reads the partial group)
        for k, (L, _, _) in enumerate(cases):
            assert want[k]["rec"]["flags"] & zsub_ref.ZDROPPED, (band, L, z)
            assert not with_table or want[k]["rec"]["lastDiag"] == bdx_ref.sweep_last_diag(band, L, z), (band, L, z)
            seen.add((want[k]["rec"]["lastDiag"] - 2) % gd)
        never, flipped = want[len(cases)]["rec"], want[len(cases) + 1]["rec"]
        assert not (never["flags"] & zsub_ref.ZDROPPED) and never["lastDiag"] == len(extra[0][0]) + len(extra[0][1]), never
        assert flipped["flags"] == zsub_ref.REACHED_END, flipped
        for k, (_, r, q, step) in enumerate(inner):
            rec = want[len(cases) + 2 + k]["rec"]
            assert rec["flags"] & zsub_ref.ZDROPPED, (band, z, k)
            assert not with_table or bdx_ref.phase_of(len(q), len(r), band, rec["lastDiag"] - 2) == ("interior", step), (band, z, k, rec)
        if band <= 64:  # the matrix batch admits these pairs
            _same_as_matrix(got, _matrix_batch(gpu, sb, BAXT, band, z, bdx_ref.SWEEP_E, table, code), (band, z))
    if with_table and band not in (15, 16):
        assert len(seen) == gd, (band, sorted(seen))  # (bands 15, 16 and 64 share C = 1: tests/test_bdx_oracle.py checks their union)
    # Z = 4 drops every pair on anti-diagonal 1 (6 > 4 + 1): nothing is stored, the end cell is (0, 0)
    _, got, want = _check(gpu, zs, sb, BAXT, band, 4, bdx_ref.SWEEP_E, table, code, picks=(0, sb.num_pairs - 1))
    assert all(r["rec"]["lastDiag"] in (1, 3) and r["rec"]["flags"] == zsub_ref.ZDROPPED for r in want)
    assert all(r["end"] == (0, 0) for r in want)


# ---- 3. both band parities and every C without a drop ----
def _related(rng, n, m, subs=0.08):
    ref = rng.integers(0, 4, n)
    q = np.resize(ref, m).copy()
    hit = rng.random(m) < subs
    q[hit] = rng.integers(0, 4, int(hit.sum()))
    if m > 30:  # one short deletion and one insertion
        q = np.concatenate([q[:10], q[12:m // 2], rng.integers(0, 4, 2), q[m // 2:]])[:m]
    return ACGT[ref].tobytes(), ACGT[np.resize(q, m)].tobytes()


@pytest.mark.parametrize("mode", ["banw_table", "baxt_table", "baxt_bonus", "baxt_huge_z"])
@pytest.mark.parametrize("band", [1, 2, 63, 64, 65, 128, 129, 256, 257, 512])
def test_bands_without_a_drop(gpu, zs, band, mode):
    rng = np.random.default_rng(300 + band)
    L = band + 45
    sizes = [(L, L), (L + min(band - 1, 1), L), (L, L + min(band - 1, 7))]
    texts = [_related(rng, n, m) for n, m in sizes]
    texts[1] = (texts[1][0], texts[1][1][:-1] + (b"A" if texts[1][1][-1:] != b"A" else b"C"))  # a mismatch at the query's end
    sb = from_strings(texts)
    algo = BANW if mode == "banw_table" else BAXT
    z, e = ((1 << 30), 5) if mode == "baxt_huge_z" else (-1, 5) if mode == "baxt_bonus" else (-1, -1)
    table, code = (TABLE, CODE) if mode.endswith("table") else (None, None)
    d, got, want = _check(gpu, zs, sb, algo, band, z, e, table, code)
    if z >= 0 or e >= 0:
        assert all(not (r["rec"]["flags"] & zsub_ref.ZDROPPED) and r["rec"]["lastDiag"] == len(sb.ref(p)) + len(sb.qry(p)) for p, r in enumerate(want))


# ---- 4. past the matrix batch's limits ----
def test_scores_past_int16(gpu, zs):
    """table entries of 100 .. 127 on related pairs of about 700 bases: scores pass 32 767, the matrix batch refuses the table"""
    rng = np.random.default_rng(44)
    table = rng.integers(100, 128, (5, 5)).astype(np.int8)
    np.fill_diagonal(table, 127)
    sb = from_strings([_related(rng, 700, 690), _related(rng, 705, 700), _related(rng, 650, 660)])
    for algo in (BANW, BAXT):
        with gpu.Batch(algo, sb.sequences, sb.pairs, *MM, *GAPS, band=64) as mb:
            assert _status(gpu, mb.set_substitution, table, CODE) == RANGE
    with gpu.Batch(BAXT, sb.sequences, sb.pairs, *MM, *GAPS, band=64) as mb:
        assert _status(gpu, mb.set_extension_table, 50, 5, table, CODE) == RANGE
    for mode in (MODES[0], MODES[1], MODES[5]):
        algo, z, e, tab, cod = _mode_args(mode, 50, 5, table, CODE)
        _, got, want = _check(gpu, zs, sb, algo, 64, z, e, tab, cod)
        assert min(r["score"] for r in want) > 32767, [r["score"] for r in want]


@pytest.mark.parametrize("z", [1 << 20, 300], ids=["never-dropping", "dropping-late"])
def test_a_pair_of_33000_bases(gpu, bo, z):
    """m + n > 65 535, one-wave workgroups; a related prefix of 30 000 bases and an unrelated tail.  Records and results against
    tests/bdx_oracle.c; the lines by rescoring them: they start at (0, 0), end at the chosen end cell and sum to the reported score."""
    rng = np.random.default_rng(33)
    pre = rng.integers(0, 4, 30000)
    q = pre.copy()
    hit = rng.random(len(q)) < 0.05
    q[hit] = rng.integers(0, 4, int(hit.sum()))
    ref = ACGT[np.concatenate([pre, rng.integers(0, 4, 3000)])].tobytes()
    qry = ACGT[np.concatenate([q, rng.integers(0, 4, 3100)])].tobytes()
    sb = from_strings([(ref, qry), (ref[:900], qry[:800])])
    want = [bo.fill(sb.ref(p), sb.qry(p), TABLE, CODE, *GAPS, 16, True, z, 5) for p in range(2)]
    assert bool(want[0]["rec"]["flags"] & zsub_ref.ZDROPPED) == (z == 300) and (z != 300 or want[0]["rec"]["lastDiag"] > 60000), want[0]
    with gpu.Batch(BAXT, sb.sequences, sb.pairs, *MM, *GAPS, band=16, flags=gpu.KEEP_BAND_DIRECTIONS) as b:
        b.set_direction_scoring(z, 5, TABLE, CODE)
        d = b.describe()
        _ran_bdx(d, BAXT, 16, z, 5, 5)
        assert d["waves_per_workgroup"] == 1, d
        b.fill()
        scores, rows, cols = b.results()
        recs = _records(b)
        for p, r in enumerate(want):
            assert recs[p] == r["rec"], (p, recs[p], r["rec"])
            assert (scores[p], (rows[p], cols[p])) == (r["score"], r["end"]), p
            lines = tuple(x.encode("latin-1") for x in b.traceback(p))
            assert bdx_ref.rescore(lines, TABLE, CODE, *GAPS) == (r["score"], r["end"][0], r["end"][1]), p
            assert lines[0].replace(b"_", b"") == sb.ref(p)[:r["end"][1]] and lines[2].replace(b"_", b"") == sb.qry(p)[:r["end"][0]], p


# ---- 5. stale pool bytes ----
def test_stale_pool_bytes_reach_nothing(gpu, zs):
    band = 100
    sb = from_strings([(r, q) for _, r, q in bdx_ref.sweep_cases(band)][:8] + [(b"ACGTACGT", b"ACGAACGT")])
    want = _want(zs, sb, BAXT, band, 7, 5, TABLE, CODE, GAPS)
    assert sum(bool(r["rec"]["flags"] & zsub_ref.ZDROPPED) for r in want) == 8
    seen = []
    with gpu.Batch(BAXT, sb.sequences, sb.pairs, *MM, *GAPS, band=band, flags=gpu.KEEP_BAND_DIRECTIONS) as b:
        b.set_direction_scoring(7, 5, TABLE, CODE)
        for byte in (0xFF, 0x5A):
            poison.poison(b, byte)
            b.fill()
            got = _observe(gpu, b)
            _against(got, want, ("poison", byte), True)
            seen.append(got)
    for key in ("scores", "ends", "lines", "recs", "text", "cigar"):
        assert seen[0][key] == seen[1][key], key
    for p in seen[0]["dirs"]:
        assert all(np.array_equal(x, y) for x, y in zip(seen[0]["dirs"][p], seen[1]["dirs"][p])), p


# ---- 6. state rules ----
def test_statuses_and_refusals_change_nothing(gpu):
    rng = np.random.default_rng(5)
    sb = from_strings([_related(rng, 90, 80), _related(rng, 70, 75)])
    lib = gpu.load()
    t8 = np.ascontiguousarray(TABLE, np.int8)
    raw = lambda b, z, e, s, a, c: lib.dpx_batch_set_direction_scoring(b._h if b is not None else None, z, e, s, a, c)
    assert raw(None, 5, 5, None, 0, None) == INVALID
    with gpu.Batch(BAXT, sb.sequences, sb.pairs, *MM, *GAPS, band=20, flags=gpu.KEEP_BAND_DIRECTIONS) as b:
        b.set_direction_scoring(20, 5, TABLE, CODE)
        before = b.describe()
        bad = CODE.copy()
        bad[7] = 5
        for args in ((-2, 5, None, 0, None), (5, -2, None, 0, None), ((1 << 30) + 1, 5, None, 0, None), (5, (1 << 30) + 1, None, 0, None),
                     (5, 5, t8.ctypes.data, 0, CODE.ctypes.data), (5, 5, t8.ctypes.data, 33, CODE.ctypes.data), (5, 5, t8.ctypes.data, 5, None),
                     (5, 5, t8.ctypes.data, 5, bad.ctypes.data)):
            assert raw(b, *args) == INVALID, args
            assert b.describe() == before
        # the three old setters keep refusing such a batch
        assert _status(gpu, b.set_extension, 7, 7) == UNSUPPORTED and _status(gpu, b.set_substitution, TABLE, CODE) == UNSUPPORTED
        assert _status(gpu, b.set_extension_table, 7, 7, TABLE, CODE) == UNSUPPORTED
        assert b.describe() == before
        b.set_direction_scoring(1 << 30, 1 << 30, TABLE, CODE)  # the largest legal values
        b.set_direction_scoring(-1, -1, None, bad)              # scores == NULL: alphabet and codeOf are ignored
        assert b.describe()["kernel"] == "k_bdir_fill"
    # not a band-direction batch: matrix and score-only batches, other algorithms, a covering BANW band (k_affine_dir)
    others = [(BAXT, 20, 0), (BAXT, 20, gpu.SCORE_ONLY), (BANW, 20, 0), (2, 0, gpu.KEEP_DIRECTIONS), (1, 0, 0), (5, 20, 0), (BANW, 200, gpu.KEEP_BAND_DIRECTIONS)]
    for algo, band, flags in others:
        with gpu.Batch(algo, sb.sequences, sb.pairs, *MM, *GAPS, band=band, flags=flags or gpu.KEEP_MATRICES) as o:
            before = o.describe()
            assert before["kernel"] != "k_bdir_fill"
            assert _status(gpu, o.set_direction_scoring, -1, -1, TABLE, CODE) == UNSUPPORTED, (algo, band, flags)
            assert _status(gpu, o.set_direction_scoring, -1, -1, None, None) == UNSUPPORTED, (algo, band, flags)
            assert o.describe() == before
    # BANW takes a table only
    with gpu.Batch(BANW, sb.sequences, sb.pairs, *MM, *GAPS, band=20, flags=gpu.KEEP_BAND_DIRECTIONS) as b:
        before = b.describe()
        for z, e in ((5, -1), (-1, 0), (5, 5)):
            assert _status(gpu, b.set_direction_scoring, z, e, TABLE, CODE) == UNSUPPORTED and _status(gpu, b.set_direction_scoring, z, e) == UNSUPPORTED
        assert b.describe() == before
        b.set_direction_scoring(-1, -1, TABLE, CODE)
        assert b.describe()["kernel"] == "k_bdx_fill"


def test_lds_and_range_refusals(gpu):
    """one wave's staged strings (align16(m + 96) + align16(n + 144) bytes) fit the 160 KiB of a workgroup, with the 1280-byte table image
    they do not: a table is refused, the scan alone is not.  And the range check: created with a positive gap open so that the bound
    of the creation's own check is within 127 * 50 000 of 2^28, the batch is refused a table whose largest entry is 127."""
    m = 81300
    assert -(-(m + 96) // 16) * 16 + -(-(m + 144) // 16) * 16 <= 160 * 1024 < -(-(m + 96) // 16) * 16 + -(-(m + 144) // 16) * 16 + 1280
    seq = np.frombuffer(b"ACGT" * ((2 * m) // 4 + 1), np.uint8)[:2 * m].copy()
    pairs = np.zeros(1, gpu.capi.PAIR_DTYPE)
    pairs[0] = (0, m, m, m)
    with gpu.Batch(BAXT, seq, pairs, *MM, *GAPS, band=16, flags=gpu.KEEP_BAND_DIRECTIONS) as b:
        before = b.describe()
        assert before["kernel"] == "k_bdir_fill" and before["waves_per_workgroup"] == 1
        assert _status(gpu, b.set_direction_scoring, 20, 5, TABLE, CODE) == UNSUPPORTED
        assert b.describe() == before
        b.set_direction_scoring(20, 5)
        assert b.describe()["kernel"] == "k_bdx_fill"
    m = 50000
    seq = np.frombuffer(b"ACGT" * (2 * m // 4), np.uint8).copy()
    pairs[0] = (0, m, m, m)
    with gpu.Batch(BAXT, seq, pairs, 1, -1, 2650, -1, band=16, flags=gpu.KEEP_BAND_DIRECTIONS) as b:  # 1 * 50 000 + 2650 * 100 000 + 2650 <= 2^28
        before = b.describe()
        big = np.full((5, 5), 127, np.int8)
        assert _status(gpu, b.set_direction_scoring, -1, -1, big, CODE) == RANGE
        assert _status(gpu, b.set_direction_scoring, 20, 5, big, CODE) == RANGE
        assert b.describe() == before
        b.set_direction_scoring(-1, -1, np.full((5, 5), 1, np.int8), CODE)
        assert b.describe()["kernel"] == "k_bdx_fill"


def test_changes_between_fills(gpu, zs):
    """NOT_FILLED follows a change and only a change; extensions after a fill without the scan; everything off is k_bdir_fill again with
    a fresh plain batch's results; Z, E and the table change between fills of one batch"""
    rng = np.random.default_rng(17)
    texts = [_related(rng, 150, 140), _related(rng, 90, 100)] + [(r, q) for _, r, q in bdx_ref.sweep_cases(64)[:3]]
    sb = from_strings(texts)
    band = 24
    t2 = TABLE.T.copy()
    calls = lambda b: (b.results, b.extensions, lambda: b.traceback(0), lambda: b.directions(0, 0), lambda: b.output_begin(0), b.cigars_begin)
    with gpu.Batch(BAXT, sb.sequences, sb.pairs, *MM, *GAPS, band=band, flags=gpu.KEEP_BAND_DIRECTIONS) as b:
        b.fill()
        plain = _observe(gpu, b, scan=False)
        assert plain["recs"] == UNSUPPORTED
        b.set_direction_scoring(-1, -1)  # nothing changed: the fill stays valid
        assert _status(gpu, b.results) == 0
        steps = [(7, 5, TABLE, CODE), (12, 5, TABLE, CODE), (12, -1, TABLE, CODE), (-1, 5, TABLE, CODE), (-1, 5, t2, CODE), (-1, -1, t2, CODE), (12, 5, None, None),
                 (-1, 0, None, None), (7, 5, TABLE, CODE)]
        for z, e, table, code in steps:
            b.set_direction_scoring(z, e, table, code)
            for call in calls(b):
                assert _status(gpu, call) == NOT_FILLED, (z, e)
            _ran_bdx(b.describe(), BAXT, band, z, e, 0 if table is None else 5)
            b.fill()
            scan = z >= 0 or e >= 0
            got = _observe(gpu, b, (0, 2, 4), scan)
            _against(got, _want(zs, sb, BAXT, band, z, e, table, code, GAPS), ("step", z, e, table is not None), scan)
            b.set_direction_scoring(z, e, table, code)  # the same settings again: nothing is invalidated
            assert _status(gpu, b.results) == 0
        b.set_direction_scoring()
        assert b.describe()["kernel"] == "k_bdir_fill" and _status(gpu, b.results) == NOT_FILLED
        b.fill()
        again = _observe(gpu, b, scan=False)
    for key in ("scores", "ends", "lines", "recs", "text", "cigar"):
        assert plain[key] == again[key], key
    for p in plain["dirs"]:
        assert all(np.array_equal(x, y) for x, y in zip(plain["dirs"][p], again["dirs"][p])), p


# ---- 7. plumbing ----
def test_plumbing_equals_the_matrix_batch(gpu, zs):
    """band 32, 50 related pairs: repeated fills on a caller's stream, packed2 input, DPX_TIME_FILLS, dpx_batch_fill_timed, the text
    pipeline and the CIGAR records, against the oracle and the matrix batch"""
    rng = np.random.default_rng(70)
    texts = []
    for k in range(50):
        n = int(rng.integers(20, 200))
        ref, q = _related(rng, n + int(rng.integers(0, 40)), n)
        texts.append((ref + ACGT[rng.integers(0, 4, int(rng.integers(0, 50)))].tobytes(), q + ACGT[rng.integers(0, 4, int(rng.integers(0, 50)))].tobytes()))
    sb = from_strings(texts)
    hip = C.CDLL("libamdhip64.so")
    handle = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(handle), 1) == 0 and handle.value   # hipStreamNonBlocking
    pk, al = gpu.pack2(sb.sequences, sb.pairs)
    z, e = 20, 5
    other = _matrix_batch(gpu, sb, BAXT, 32, z, e, TABLE, CODE)
    want = _want(zs, sb, BAXT, 32, z, e, TABLE, CODE, GAPS)
    assert 5 <= sum(bool(r["rec"]["flags"] & 1) for r in want) <= 48

    def three_fills_on_the_stream(b):
        for _ in range(3):
            b.fill(handle.value)

    def timed(b):
        usec = C.c_double(0.0)
        assert gpu.load().dpx_batch_fill_timed(b._h, 2, C.byref(usec)) == 0 and usec.value > 0

    for kw, fill in (({}, three_fills_on_the_stream), ({"packed2": (pk, al, sb.sequences.size)}, None), ({}, timed)):
        d, got, _ = _check(gpu, zs, sb, BAXT, 32, z, e, TABLE, CODE, want=want, picks=range(0, 50, 7), fill=fill, **kw)
        assert d["seq_input"] == ("packed2" if kw else "bytes")
        _same_as_matrix(got, other, tuple(kw))
    with gpu.Batch(BAXT, sb.sequences, sb.pairs, *MM, *GAPS, band=32, flags=gpu.KEEP_BAND_DIRECTIONS | gpu.TIME_FILLS) as b:
        b.set_direction_scoring(z, e, TABLE, CODE)
        b.fill(handle.value)
        usec = C.c_double(0.0)
        assert gpu.load().dpx_batch_last_fill_usec(b._h, C.byref(usec)) == 0 and usec.value > 0
        _same_as_matrix(_observe(gpu, b, ()), other, "timed fills")
    assert hip.hipStreamDestroy(handle) == 0
