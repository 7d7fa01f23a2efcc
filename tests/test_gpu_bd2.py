"""Two-piece band-direction batches (DPX_KEEP_BAND_DIRECTIONS | DPX_TWO_PIECE_GAPS, k_bd2_fill / k_bd2_traceback / k_bd2_export) on the
GPU, bit-exact against tests/bd2_oracle.c (int64, band only): every result, record, line, CIGAR, text block and all six exported planes,
masked behind lastDiag.  tests/test_bd2_oracle.py checks that oracle against the one-piece oracles and against a gap-length-enumerating
DP.  Modes without a table score by params.match / params.mismatch; the oracle is then given the table that scores as byte equality
does.  Every case asserts from dpx_batch_describe that k_bd2_fill ran."""
import re

import numpy as np
import pytest

import bd2_ref
import bdx_ref
import cigar_ref
import poison
import zsub_ref
from bd2_ref import BANW, BAXT, MODES
from dpx_gpu_genomics_project_amd.synth import from_strings

pytestmark = pytest.mark.gpu

INVALID, RANGE, NOT_FILLED, NO_MATRIX, UNSUPPORTED = -1, -4, -6, -7, -8
TABLE, CODE = zsub_ref.acgtn_table()
MM = (2, -4)
P1, P2 = (-4, -2), (-24, -1)  # the crossover is at k = 20
ACGT = np.frombuffer(b"ACGT", np.uint8)
NAME = {BANW: "BANW", BAXT: "BAXT"}
BANDS = [1, 2, 33, 64, 65, 128, 129, 255, 256]  # every C, both parities, the C boundaries


@pytest.fixture(scope="module")
def orc(tmp_path_factory):
    return bd2_ref.build(tmp_path_factory.mktemp("bd2_gpu"))


def _flags(gpu):
    return gpu.KEEP_BAND_DIRECTIONS | gpu.TWO_PIECE_GAPS


def _status(gpu, call, *args):
    try:
        call(*args)
    except gpu.DpxError as e:
        return e.status
    return 0


def _ran_bd2(d, algo, band, z, e, alphabet, p2):
    assert d["algo"] == NAME[algo] and d["kernel_algo"] == NAME[algo] and d["kernel"] == "k_bd2_fill", d
    assert d["traceback"] == "k_bd2_traceback" and d["matrix"] == "banddir8" and d["dtype"] == "int32", d
    assert d["rows_per_lane"] == bd2_ref.cpl(band) and d["gap2"] == "%d,%d" % p2, d
    assert (d.get("zdrop"), d.get("end_bonus")) == ((z, e) if (z >= 0 or e >= 0) else (None, None)), d
    assert d.get("subst") == (alphabet or None), d


def _records(b):
    return [{k: int(r[k]) for k in zsub_ref.FIELDS} for r in b.extensions()]


def _observe(gpu, b, picks="all", scan=True, which=range(6)):
    """everything a filled two-piece batch reports"""
    scores, rows, cols = b.results()
    out = {"scores": scores.tolist(), "ends": list(zip(rows.tolist(), cols.tolist())),
           "lines": [tuple(x.encode("latin-1") for x in b.traceback(p)) for p in range(b.num_pairs)]}
    out["recs"] = _records(b) if scan else _status(gpu, b.extensions)
    b.output_begin(5)
    out["text"] = b.output_end()[0]
    b.cigars_begin(gpu.CIGAR_EXTENDED)
    recs, ops = b.cigars_end()
    out["cigar"] = (recs.tobytes(), ops.tolist())
    out["cigar_recs"], out["cigar_ops"] = recs, ops
    picks = range(b.num_pairs) if picks == "all" else picks
    out["dirs"] = {p: [b.directions(p, w) for w in which] for p in picks}
    return out


def _against(gpu, got, want, tag, scan):
    for p, r in enumerate(want):
        if scan:
            assert got["recs"][p] == r["rec"], (tag, p, got["recs"][p], r["rec"])
        assert (got["scores"][p], got["ends"][p]) == (r["score"], r["end"]), (tag, p, got["scores"][p], got["ends"][p], r["score"], r["end"])
        assert got["lines"][p] == r["lines"], (tag, p)
        rec = got["cigar_recs"][p]  # the CIGAR is the lines', run for run: it does not say which piece paid for a gap
        ops = got["cigar_ops"][int(rec["opsOffset"]):int(rec["opsOffset"]) + int(rec["numOps"])]
        wrec, wops = cigar_ref.records_and_ops(r["lines"], *r["end"])
        assert ops.tolist() == wops and {k: int(rec[k]) for k in wrec} == wrec, (tag, p)
    if not scan:
        assert got["recs"] == UNSUPPORTED, tag  # a fill that did not run the scan has no records
    assert len(want) == len(got["scores"]) > 0 and got["dirs"] and all(len(v) == 6 for v in got["dirs"].values()), tag  # (nothing compares empty)
    for p, planes in got["dirs"].items():
        for key, have, exp in zip(("H", "I", "D", "I2", "D2", "PIECE"), planes, want[p]["dirs"]):
            assert np.array_equal(have, exp), (tag, p, key, want[p]["rec"], np.argwhere(have != exp)[:4])
    assert got["text"] == b"".join(b"%d | %d\n" % (5 + p, r["score"]) + b"".join(x + b"\n" for x in r["lines"]) for p, r in enumerate(want)), tag


def _want(orc, sb, algo, band, z, e, table, code, p1, p2, mm=MM, used=b"ACGTN", **kw):
    t, c = (np.asarray(table, np.int8), code) if table is not None else bdx_ref.byte_table(*mm, used)
    return [orc.expect(sb.ref(p), sb.qry(p), t, c, p1, p2, band, algo == BAXT, z, e, **kw) for p in range(sb.num_pairs)]


def _check(gpu, orc, sb, algo, band, z=-1, e=-1, table=None, code=None, p1=P1, p2=P2, mm=MM, used=b"ACGTN", picks="all"):
    """one two-piece batch in one mode against the oracle; returns (observations, expectations)"""
    want = _want(orc, sb, algo, band, z, e, table, code, p1, p2, mm, used)
    scan = z >= 0 or e >= 0
    with gpu.Batch(algo, sb.sequences, sb.pairs, *mm, *p1, band=band, flags=_flags(gpu)) as b:
        b.set_second_gap(*p2)
        if scan or table is not None:
            b.set_direction_scoring(z, e, table, code)
        _ran_bd2(b.describe(), algo, band, z, e, 0 if table is None else np.asarray(table).shape[0], p2)
        b.fill()
        assert _status(gpu, b.matrix, 0) == NO_MATRIX
        got = _observe(gpu, b, picks, scan)
    _against(gpu, got, want, (NAME[algo], band, z, e, table is not None, p1, p2), scan)
    return got, want


def _mode_args(mode, z, e):
    _, algo, with_table, drop, bonus = mode
    return algo, (z if drop else -1), (e if bonus else -1), (TABLE if with_table else None), (CODE if with_table else None)


def _related(rng, n, gaps=(), subs=0.06):
    """(ref, qry): the query is the reference with substitutions and, per (position fraction, length, kind) of `gaps`, a planted indel"""
    ref = rng.integers(0, 4, n)
    q = ref.copy()
    hit = rng.random(n) < subs
    q[hit] = rng.integers(0, 4, int(hit.sum()))
    for frac, length, kind in sorted(gaps, reverse=True):
        at = int(frac * n)
        q = np.concatenate([q[:at], q[at + length:]]) if kind == "D" else np.concatenate([q[:at], rng.integers(0, 4, length), q[at:]])
    return ACGT[ref].tobytes(), ACGT[q].tobytes()


# ---- 1. every band class, all eight modes ----
@pytest.mark.parametrize("band", BANDS)
def test_bands(gpu, orc, band):
    rng = np.random.default_rng(700 + band)
    L = band + 45
    g = min(band - 1, 30)  # an indel long enough for piece 2 where the band admits it
    texts = [_related(rng, L), _related(rng, L + 21, [(0.4, g, "D")]), _related(rng, L, [(0.5, g, "I")]),
             _related(rng, L + 3, [(0.3, min(g, 3), "D"), (0.7, min(g, 2), "I")])]
    texts[0] = (texts[0][0], texts[0][1][:-1] + (b"A" if texts[0][1][-1:] != b"A" else b"C"))  # a mismatch at the query's end
    for mode in MODES:
        algo, z, e, table, code = _mode_args(mode, 1 << 30 if band % 2 else 60, 5)
        keep = [t for t in texts if algo == BAXT or abs(len(t[0]) - len(t[1])) < band]
        _check(gpu, orc, from_strings(keep), algo, band, z, e, table, code)


# ---- 2. the fuzz: m, n in 0..90 with the edge sizes of the group layout, per mode ----
FUZZ_PIECES = [((-3, -2), (-7, -1)), ((-7, -1), (-3, -2)), ((0, -3), (-6, 0)), ((-2, -1), (-2, -1))]
FUZZ_BANDS = [1, 2, 7, 16, 33, 70, 129]


def _fuzz_texts(band):
    rng = np.random.default_rng(4000 + band)
    gd = bd2_ref.gd(band)
    sizes = [(0, 0), (0, 5), (6, 0), (1, 1), (1, 0), (0, 1), (1, band + 3), (band + 2, 2), (90, 90), (90, 1)]
    for k in (1, 2, 5):  # m + n - 1 at a multiple of Gd and one to either side
        for d in (-1, 0, 1):
            total = k * gd + 1 + d
            sizes.append((total // 2, total - total // 2))
    sizes += [(int(rng.integers(0, 91)), int(rng.integers(0, 91))) for _ in range(14)]
    texts = []
    for n, m in sizes:
        ref = rng.integers(0, 4, n)
        qry = np.resize(ref, m).copy() if n else rng.integers(0, 4, m)
        hit = rng.random(m) < 0.15
        qry[hit] = rng.integers(0, 4, int(hit.sum()))
        if m > 24:
            qry = np.concatenate([qry[:8], qry[8 + int(rng.integers(1, 9)):]])
            qry = np.concatenate([qry, rng.integers(0, 4, m - len(qry))])
        texts.append((ACGT[ref].tobytes(), ACGT[qry].tobytes()))
    return texts


@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_fuzz(gpu, orc, mode):
    for k, band in enumerate(FUZZ_BANDS):
        texts = _fuzz_texts(band)
        algo, z, e, table, code = _mode_args(mode, (0, 9, 25)[k % 3], 3)
        if algo == BANW:
            texts = [t for t in texts if abs(len(t[0]) - len(t[1])) < band]
        else:
            assert any(abs(len(t[0]) - len(t[1])) >= band for t in texts) or band > 90
        p1, p2 = FUZZ_PIECES[k % len(FUZZ_PIECES)]
        _check(gpu, orc, from_strings(texts), algo, band, z, e, table, code, p1, p2)


# ---- 3. the crossover at k = 20 ----
def test_crossover(gpu, orc):
    rng = np.random.default_rng(20)
    texts = []
    for k, length in enumerate((19, 20, 21, 70, 150, 19, 20, 21, 70, 150)):
        texts.append(_related(rng, 300 + 40 * k, [(0.45, length, "D" if k < 5 else "I")], subs=0.03))
    texts.append(_related(rng, 700, [(0.2, 70, "D"), (0.6, 150, "I")], subs=0.03))
    sb = from_strings(texts)
    table, code = bdx_ref.byte_table(*MM, b"ACGTN")
    for algo, band in ((BANW, 200), (BAXT, 256), (BAXT, 128)):
        two = _want(orc, sb, algo, band, -1, -1, None, None, P1, P2, planes=False, lines=False)
        one = _want(orc, sb, algo, band, -1, -1, None, None, P1, P1, planes=False, lines=False)
        # the condition, on the oracle alone: the second piece changes the score of at least a quarter of the pairs
        assert sum(t["score"] > o["score"] for t, o in zip(two, one)) * 4 >= len(texts), (band, [(t["score"], o["score"]) for t, o in zip(two, one)])
        got, want = _check(gpu, orc, sb, algo, band, picks=(0, 3, 10))
        for p, r in enumerate(want):  # the lines rescore under the two pieces to the reported score
            assert bd2_ref.rescore(got["lines"][p], table, code, P1, P2) == (r["score"], *r["end"]), (band, p)
        runs = [len(x) for r in want for x in re.findall(rb"_+", r["lines"][0] + b" " + r["lines"][2])]
        assert max(runs) > 64  # a gap run longer than one ballot, and than the ring's half at C = 4


# ---- 4. identity: equal pieces are the unflagged band-direction batch ----
def _bdir_batch(gpu, sb, algo, band, z, e, table, code, p1):
    with gpu.Batch(algo, sb.sequences, sb.pairs, *MM, *p1, band=band, flags=gpu.KEEP_BAND_DIRECTIONS) as b:
        if z >= 0 or e >= 0 or table is not None:
            b.set_direction_scoring(z, e, table, code)
        assert b.describe()["matrix"] == "banddir4"
        b.fill()
        return _observe(gpu, b, "all", z >= 0 or e >= 0, which=range(3))


@pytest.mark.parametrize("band", [16, 100, 200])
def test_identity_with_equal_pieces(gpu, band):
    rng = np.random.default_rng(band)
    texts = [_related(rng, band + 40, [(0.5, min(band - 1, 9), "D")]), _related(rng, band + 30, [(0.3, 4, "I")]), _related(rng, 50),
             (b"", b"ACG"), (b"ACGT", b"")]
    texts += [(r, q) for _, r, q in bdx_ref.sweep_cases(band)[:3]]
    p1 = zsub_ref.GAPS
    for mode in MODES:
        algo, z, e, table, code = _mode_args(mode, 7, 5)
        sb = from_strings([t for t in texts if algo == BAXT or abs(len(t[0]) - len(t[1])) < band])
        base = _bdir_batch(gpu, sb, algo, band, z, e, table, code, p1)
        for setter in (False, True):
            with gpu.Batch(algo, sb.sequences, sb.pairs, *MM, *p1, band=band, flags=_flags(gpu)) as b:
                if setter:
                    b.set_second_gap(*p1)
                if z >= 0 or e >= 0 or table is not None:
                    b.set_direction_scoring(z, e, table, code)
                assert b.describe()["kernel"] == "k_bd2_fill" and b.describe()["gap2"] == "%d,%d" % p1
                b.fill()
                got = _observe(gpu, b, "all", z >= 0 or e >= 0)
            for key in ("scores", "ends", "recs", "lines", "text", "cigar"):
                assert got[key] == base[key], (mode[0], band, setter, key)
            for p in base["dirs"]:
                for w in range(3):
                    assert np.array_equal(got["dirs"][p][w], base["dirs"][p][w]), (mode[0], band, setter, p, w)
                assert np.array_equal(got["dirs"][p][3], got["dirs"][p][1]) and np.array_equal(got["dirs"][p][4], got["dirs"][p][2]), (mode[0], p)


# ---- 5. one long pair past the matrix batch's limits ----
def test_long_pair(gpu, orc):
    rng = np.random.default_rng(2030)
    ref, qry = _related(rng, 20300, [(0.15, 100, "D"), (0.3, 250, "I"), (0.5, 180, "D"), (0.7, 120, "I"), (0.85, 250, "D")], subs=0.02)
    qry = qry[:20000]
    assert (len(ref), len(qry)) == (20300, 20000)
    sb = from_strings([(ref, qry)])
    z, e, band = 400, 5, 256
    with pytest.raises(gpu.DpxError) as refused:
        gpu.Batch(BAXT, sb.sequences, sb.pairs, *MM, *P1, band=band)
    assert refused.value.status == RANGE
    want = orc.expect(ref, qry, TABLE, CODE, P1, P2, band, True, z, e, planes=False)
    with gpu.Batch(BAXT, sb.sequences, sb.pairs, *MM, *P1, band=band, flags=_flags(gpu)) as b:
        b.set_second_gap(*P2)
        b.set_direction_scoring(z, e, TABLE, CODE)
        _ran_bd2(b.describe(), BAXT, band, z, e, 5, P2)
        b.fill()
        scores, rows, cols = b.results()
        assert (int(scores[0]), (int(rows[0]), int(cols[0]))) == (want["score"], want["end"])
        assert _records(b)[0] == want["rec"]
        lines = tuple(x.encode("latin-1") for x in b.traceback(0))
    assert lines == want["lines"]
    er, ec = want["end"]
    assert lines[0].replace(b"_", b"") == ref[:ec] and lines[2].replace(b"_", b"") == qry[:er]
    assert bd2_ref.rescore(lines, TABLE, CODE, P1, P2) == (want["score"], er, ec)
    assert want["score"] > orc.expect(ref, qry, TABLE, CODE, P1, P1, band, True, z, e, planes=False, lines=False)["score"]


# ---- 6. the z-drop sweep with unequal pieces ----
SWEEP_P2 = (-8, 0)  # the flatter piece: pen = 0


@pytest.mark.parametrize("band", [15, 16, 64, 100, 200])
def test_drop_sweep(gpu, orc, band):
    cases = bdx_ref.sweep_cases(band)[:bd2_ref.gd(band) + 2]
    inner = bdx_ref.interior_cases(band) if band in bdx_ref.INTERIOR_BANDS else []
    sb = from_strings([(r, q) for _, r, q in cases] + [(r, q) for _, r, q, _ in inner])
    seen = set()
    for z in bdx_ref.SWEEP_Z:
        got, want = _check(gpu, orc, sb, BAXT, band, z, bdx_ref.SWEEP_E, TABLE, CODE, zsub_ref.GAPS, SWEEP_P2)
        assert all(r["rec"]["flags"] & zsub_ref.ZDROPPED for r in want), (band, z)
        seen |= {((r["rec"]["lastDiag"] - 2) % bd2_ref.gd(band), r["rec"]["lastDiag"] & 1) for r in want}
    # an even anti-diagonal is the first step of a loop body (the second then does not run), an odd one the second; these pairs drop on
    # anti-diagonals of both parities at every band but 15
    assert {s[1] for s in seen} == ({1} if band == 15 else {0, 1}), (band, sorted(seen))
    assert len({s[0] for s in seen}) >= min(bd2_ref.gd(band), 4), (band, sorted(seen))  # drops at several places of a store group
    # Z = 4 drops every pair on anti-diagonal 1 (g(1) = -6, and 6 > 4 + 0): nothing is stored, the end cell is (0, 0)
    _, want = _check(gpu, orc, sb, BAXT, band, 4, bdx_ref.SWEEP_E, TABLE, CODE, zsub_ref.GAPS, SWEEP_P2, picks=(0, sb.num_pairs - 1))
    assert all(r["rec"]["lastDiag"] == 1 and r["rec"]["flags"] == zsub_ref.ZDROPPED and r["end"] == (0, 0) for r in want)


# ---- 7. stale pool bytes ----
def test_stale_pool_bytes_reach_nothing(gpu, orc):
    band = 100
    rng = np.random.default_rng(5)
    sb = from_strings([(r, q) for _, r, q in bdx_ref.sweep_cases(band)][:6] + [(b"ACGTACGT", b"ACGAACGT"), _related(rng, 160, [(0.5, 30, "D")])])
    want = _want(orc, sb, BAXT, band, 7, 5, TABLE, CODE, zsub_ref.GAPS, SWEEP_P2)
    assert sum(bool(r["rec"]["flags"] & zsub_ref.ZDROPPED) for r in want) >= 6
    seen = []
    with gpu.Batch(BAXT, sb.sequences, sb.pairs, *MM, *zsub_ref.GAPS, band=band, flags=_flags(gpu)) as b:
        b.set_second_gap(*SWEEP_P2)
        b.set_direction_scoring(7, 5, TABLE, CODE)
        for byte in (0xFF, 0x5A):
            poison.poison(b, byte)
            b.fill()
            got = _observe(gpu, b)
            _against(gpu, got, want, ("poison", byte), True)
            seen.append(got)
    for key in ("scores", "ends", "lines", "recs", "text", "cigar"):
        assert seen[0][key] == seen[1][key], key
    for p in seen[0]["dirs"]:
        assert all(np.array_equal(x, y) for x, y in zip(seen[0]["dirs"][p], seen[1]["dirs"][p])), p


# ---- 8. the plumbing of a band-direction batch: packed2 input, an explicit device, a caller's stream, timed and repeated fills ----
def test_packed2_device_stream_and_timed_fills(gpu, orc):
    import ctypes as C

    rng = np.random.default_rng(88)
    sb = from_strings([_related(rng, 400, [(0.5, 40, "D")]), _related(rng, 150, [(0.4, 25, "I")]), _related(rng, 90), (b"ACGT", b"")])
    band, z, e = 130, 80, 5
    want = _want(orc, sb, BAXT, band, z, e, TABLE, CODE, P1, P2)
    packed, alphabet = gpu.pack2(sb.sequences, sb.pairs)
    hip = C.CDLL("libamdhip64.so")
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0 and stream.value  # hipStreamNonBlocking
    for kw in (dict(packed2=(packed, alphabet, sb.sequences.size)), dict(device=0, flags=_flags(gpu) | gpu.TIME_FILLS)):
        kw.setdefault("flags", _flags(gpu))
        with gpu.Batch(BAXT, sb.sequences, sb.pairs, *MM, *P1, band=band, **kw) as b:
            b.set_second_gap(*P2)
            b.set_direction_scoring(z, e, TABLE, CODE)
            assert b.describe()["kernel"] == "k_bd2_fill" and b.describe()["seq_input"] == ("packed2" if "packed2" in kw else "bytes")
            b.fill(stream.value)  # no synchronisation between create and this fill
            _against(gpu, _observe(gpu, b), want, ("stream", sorted(kw)), True)
            assert b.fill_timed(3) > 0
            b.fill()
            _against(gpu, _observe(gpu, b), want, ("refill", sorted(kw)), True)
    assert hip.hipStreamDestroy(stream) == 0


# ---- 9. statuses and state rules ----
def test_statuses_and_refusals_change_nothing(gpu, orc):
    rng = np.random.default_rng(8)
    texts = [_related(rng, 120, [(0.5, 25, "D")]), _related(rng, 90)]
    sb = from_strings(texts)
    two = gpu.TWO_PIECE_GAPS

    def create(algo, flags, band=64, gaps=P1):
        return _status(gpu, lambda: gpu.Batch(algo, sb.sequences, sb.pairs, *MM, *gaps, band=band, flags=flags).close())

    assert create(BAXT, two) == INVALID and create(BANW, two | gpu.SCORE_ONLY) == INVALID  # 0x20 without 0x10
    assert create(gpu.ALGO_LSW, two) == INVALID
    for algo in (gpu.ALGO_LSW, gpu.ALGO_ANW, gpu.ALGO_BSW, gpu.ALGO_BASW):
        assert create(algo, _flags(gpu)) == UNSUPPORTED, algo
    assert create(BAXT, _flags(gpu), band=257) == UNSUPPORTED and create(BANW, _flags(gpu), band=300) == UNSUPPORTED
    assert create(BAXT, _flags(gpu), band=256) == 0 and create(BANW, _flags(gpu), band=256) == 0
    with gpu.Batch(BAXT, sb.sequences, sb.pairs, *MM, *P1, band=64, flags=gpu.KEEP_BAND_DIRECTIONS) as plain:
        before = plain.describe()
        assert _status(gpu, plain.set_second_gap, *P2) == UNSUPPORTED and plain.describe() == before
        plain.fill()
        for w in (gpu.MAT_I2, gpu.MAT_D2, gpu.MAT_H_PIECE):
            assert _status(gpu, plain.directions, 0, w) == INVALID
    with gpu.Batch(BAXT, sb.sequences, sb.pairs, *MM, *P1, band=64) as mb:
        assert _status(gpu, mb.set_second_gap, *P2) == UNSUPPORTED
    assert gpu.load().dpx_batch_set_second_gap(None, -24, -1) == INVALID

    with gpu.Batch(BANW, sb.sequences, sb.pairs, *MM, *P1, band=121, flags=_flags(gpu)) as b:  # a covering BANW band stays on the band kernel
        d = b.describe()
        assert d["kernel"] == "k_bd2_fill" and d["kernel_algo"] == "BANW" and d["gap2"] == "%d,%d" % P1, d
        assert _status(gpu, b.set_direction_scoring, 5, -1, None, None) == UNSUPPORTED  # (BANW has no extension mode)
    with gpu.Batch(BAXT, sb.sequences, sb.pairs, *MM, *P1, band=64, flags=_flags(gpu)) as b:
        before = b.describe()
        assert _status(gpu, b.results) == NOT_FILLED
        for args in (((1 << 20) + 1, -1), (-24, -(1 << 20) - 1), (-(1 << 20) - 1, 0)):
            assert _status(gpu, b.set_second_gap, *args) == RANGE and b.describe() == before, args
        for setter, args in ((b.set_extension, (5, 5)), (b.set_substitution, (TABLE, CODE)), (b.set_extension_table, (5, 5, TABLE, CODE))):
            assert _status(gpu, setter, *args) == UNSUPPORTED and b.describe() == before, setter
        b.fill()
        assert _status(gpu, b.results) == 0
        b.set_second_gap(*P1)  # the same values: nothing is invalidated
        assert _status(gpu, b.results) == 0
        # changes between fills: the piece, then a table, then everything off
        steps = [(lambda: b.set_second_gap(*P2), dict(p2=P2)), (lambda: b.set_direction_scoring(30, 5, TABLE, CODE), dict(p2=P2, z=30, e=5, table=TABLE, code=CODE)),
                 (lambda: b.set_direction_scoring(-1, -1, None, None), dict(p2=P2))]
        for change, kw in steps:
            change()
            assert _status(gpu, b.results) == NOT_FILLED and _status(gpu, b.traceback, 0) == NOT_FILLED
            assert _status(gpu, b.extensions) == NOT_FILLED and _status(gpu, b.directions, 0) == NOT_FILLED
            b.fill()
            z, e = kw.get("z", -1), kw.get("e", -1)
            want = _want(orc, sb, BAXT, 64, z, e, kw.get("table"), kw.get("code"), P1, kw["p2"])
            _against(gpu, _observe(gpu, b, "all", z >= 0), want, ("state", sorted(kw)), z >= 0)
    # the range check runs on both componentwise bounds of the two pieces
    big = from_strings([(b"A" * 3000, b"A" * 3000)])
    with gpu.Batch(BAXT, big.sequences, big.pairs, 1, -1, -4, -2, band=256, flags=_flags(gpu)) as b:
        before = b.describe()
        assert _status(gpu, b.set_second_gap, -(1 << 20), -(1 << 20)) == RANGE and b.describe() == before  # 255 * 2^20 passes 2^28
        assert _status(gpu, b.set_second_gap, -24, 1 << 17) == RANGE and b.describe() == before  # 6000 * 2^17 passes 2^28 upwards
        assert _status(gpu, b.set_second_gap, -24, -1) == 0
