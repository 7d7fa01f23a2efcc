"""DPX_LONG_SCORES on the GPU, through the C ABI: the int32 band fills with nothing stored but the results (k_bscore_fill on BANW / BAXT,
k_lscore_fill on BSW / BASW).  Every case asserts from dpx_batch_describe that the score-only kernel ran -- on a library that predates the
flag the bit is ignored, describe says k_bdir_fill / k_bdl_fill and dpx_batch_directions succeeds -- and compares score, end row and end
column with the direction batch of the same pairs (DPX_KEEP_BAND_DIRECTIONS / DPX_KEEP_LOCAL_BAND_DIRECTIONS without the bit) and with
the int64 band-only CPU oracles (tests/bdx_oracle.c, bdl_oracle.c, bdlt_oracle.c); in extension mode the dpx_extension records too.
Inputs and expectations: tests/bscore_cases.py."""
import ctypes as C

import numpy as np
import pytest

import bscore_cases as bc
from bscore_cases import ALGOS, BANDS, BANW, BASW, BAXT, BSW, KERNEL, NAME, W
from bdx_ref import cpl
from dpx_gpu_genomics_project_amd.synth import from_strings
from zext_ref import FIELDS

pytestmark = pytest.mark.gpu

INVALID, RANGE, NOT_FILLED, NO_MATRIX, UNSUPPORTED = -1, -4, -6, -7, -8
TABLE_GAPS = (0, 0, -5, -1)  # match / mismatch are not read under a table


@pytest.fixture(scope="module")
def orc(tmp_path_factory):
    return bc.Oracles(tmp_path_factory.mktemp("bscore_gpu"))


def _storage(gpu, algo):
    return gpu.KEEP_LOCAL_BAND_DIRECTIONS if bc.is_local(algo) else gpu.KEEP_BAND_DIRECTIONS


def _status(gpu, call, *args, **kw):
    try:
        call(*args, **kw)
    except gpu.DpxError as e:
        return e.status
    return 0


def _apply(b, algo, table, z, e):
    """the one admitted scoring setter of the batch's family, when there is something to set"""
    if bc.is_local(algo):
        if table is not None:
            b.set_local_direction_table(*table)
    elif table is not None or z >= 0 or e >= 0:
        b.set_direction_scoring(z, e, *(table if table is not None else (None, None)))


def _results(b, scan):
    s, r, c = b.results()
    out = {"scores": s.tolist(), "ends": list(zip(r.tolist(), c.tolist()))}
    if scan:
        out["recs"] = [{k: int(rec[k]) for k in FIELDS} for rec in b.extensions()]
    return out


def _ran_score_only(gpu, b, algo, band, table=None, z=-1, e=-1):
    d = b.describe()
    assert (d["algo"], d["kernel_algo"], d["kernel"], d["store"], d["dtype"]) == (NAME[algo], NAME[algo], KERNEL[algo], 0, "int32"), d
    assert d["rows_per_lane"] == cpl(band) and "matrix" not in d and "traceback" not in d and d["pool_addr"] == "0x0", d
    assert d.get("subst") == (None if table is None else np.asarray(table[0]).shape[0]), d
    assert (d.get("zdrop"), d.get("end_bonus")) == ((z, e) if (z >= 0 or e >= 0) else (None, None)), d
    assert b.info()["matrix_bytes"] == 0
    assert _status(gpu, b.directions, 0) == NO_MATRIX  # (a library that ignores the bit exports the codes here)
    return d


def _long(gpu, algo, sb, band, w=W, table=None, z=-1, e=-1, mask=None, fill=None, extra_flags=0, **kw):
    """the DPX_LONG_SCORES batch of the pairs: (results, describe)"""
    with gpu.Batch(algo, sb.sequences, sb.pairs, *bc.weights(algo, w), band=band, flags=_storage(gpu, algo) | gpu.LONG_SCORES | extra_flags, **kw) as b:
        _apply(b, algo, table, z, e)
        if mask is not None:
            b.set_reversed(mask)
        d = _ran_score_only(gpu, b, algo, band, table, z, e)
        (fill or (lambda batch: batch.fill()))(b)
        return _results(b, z >= 0 or e >= 0), d


def _direction(gpu, algo, sb, band, w=W, table=None, z=-1, e=-1, mask=None):
    """the direction batch of the same pairs, as such a caller runs it without the bit"""
    with gpu.Batch(algo, sb.sequences, sb.pairs, *bc.weights(algo, w), band=band, flags=_storage(gpu, algo)) as b:
        _apply(b, algo, table, z, e)
        if mask is not None:
            b.set_reversed(mask)
        d = b.describe()
        assert d["kernel"] in bc.TWIN_KERNELS[algo] and d["store"] == 1 and d["matrix"] == "banddir4", d
        b.fill()
        assert b.info()["matrix_bytes"] > 0
        return _results(b, z >= 0 or e >= 0)


def _same(got, other, tag):
    for key in other:
        assert got[key] == other[key], (tag, key, [(p, a, b) for p, (a, b) in enumerate(zip(got[key], other[key])) if a != b][:4])


def _against_oracle(got, want, tag):
    for p, (score, end, rec) in enumerate(want):
        assert (got["scores"][p], got["ends"][p]) == (score, end), (tag, p, got["scores"][p], got["ends"][p], score, end)
        if rec is not None:
            assert got["recs"][p] == rec, (tag, p, got["recs"][p], rec)


# ---------------------------------------------------------------------------------------- 1. every band class, phase and shape

@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("algo", ALGOS, ids=[NAME[a] for a in ALGOS])
def test_equals_the_direction_batch_and_the_oracle(gpu, orc, algo, band):
    texts = bc.band_pairs(algo, band)
    sb = from_strings(texts)
    got, _ = _long(gpu, algo, sb, band)
    _same(got, _direction(gpu, algo, sb, band), (NAME[algo], band, "direction batch"))
    _against_oracle(got, orc.expect_all(algo, texts, band, w=bc.weights(algo)), (NAME[algo], band))


# ---------------------------------------------------------------------------------------- 2. tables

@pytest.mark.parametrize("algo", ALGOS, ids=[NAME[a] for a in ALGOS])
@pytest.mark.parametrize("which", ["acgtn", "wide"])
def test_tables(gpu, orc, algo, which):
    table, texts = (bc.ACGTN_TABLE, bc.acgtn_pairs()) if which == "acgtn" else (bc.WIDE_TABLE, bc.byte_pairs())
    if which == "acgtn":
        assert table[0][4, 4] < 0
    else:
        assert table[0].shape == (32, 32) and table[0].min() == -128 and table[0].max() == 127 and not np.array_equal(table[0], table[0].T)
        assert any(max(r) >= 128 for r, _ in texts)
    band = 70
    w = (2, -3) + TABLE_GAPS[2:]
    sb = from_strings(texts)
    got, _ = _long(gpu, algo, sb, band, w=w, table=table)
    _same(got, _direction(gpu, algo, sb, band, w=w, table=table), (NAME[algo], which, "direction batch"))
    want_table = orc.expect_all(algo, texts, band, w=bc.weights(algo, w), table=table)
    _against_oracle(got, want_table, (NAME[algo], which))
    # set, fill, clear, fill, set again: the results follow the setting each time
    used = bytes(sorted(set(b"".join(r + q for r, q in texts))))
    plain_ok = len(used) <= 32  # (byte equality as a table for the oracle of BANW / BAXT needs at most 32 distinct bytes)
    with gpu.Batch(algo, sb.sequences, sb.pairs, *bc.weights(algo, w), band=band, flags=_storage(gpu, algo) | gpu.LONG_SCORES) as b:
        _ran_score_only(gpu, b, algo, band)
        b.fill()
        plain = _results(b, False)
        if plain_ok or bc.is_local(algo):
            _against_oracle(plain, orc.expect_all(algo, texts, band, w=bc.weights(algo, w), used=used), (NAME[algo], which, "before"))
        _apply(b, algo, table, -1, -1)
        assert _status(gpu, b.results) == NOT_FILLED  # a changed table invalidates the fill
        _ran_score_only(gpu, b, algo, band, table)
        b.fill()
        _against_oracle(_results(b, False), want_table, (NAME[algo], which, "set"))
        _apply(b, algo, table, -1, -1)  # the same table again invalidates nothing
        _against_oracle(_results(b, False), want_table, (NAME[algo], which, "same again"))
        if bc.is_local(algo):
            b.set_local_direction_table(None)
        else:
            b.set_direction_scoring(-1, -1, None, None)
        _ran_score_only(gpu, b, algo, band)
        b.fill()
        _same(_results(b, False), plain, (NAME[algo], which, "cleared"))
        _apply(b, algo, table, -1, -1)
        b.fill()
        _against_oracle(_results(b, False), want_table, (NAME[algo], which, "set again"))
    assert plain["scores"] != got["scores"]


# ---------------------------------------------------------------------------------------- 3. extension mode

@pytest.mark.parametrize("with_table", [False, True], ids=["plain", "table"])
@pytest.mark.parametrize("z,e", [(40, -1), (-1, 10), (40, 10)], ids=["zdrop", "bonus", "both"])
def test_extension_mode(gpu, orc, with_table, z, e):
    texts = bc.extension_pairs()
    table = bc.ACGTN_TABLE if with_table else None
    w = TABLE_GAPS if with_table else W
    band = 100
    want = orc.expect_all(BAXT, texts, band, w=w, table=table, zdrop=z, end_bonus=e)
    flags = [rec["flags"] for _, _, rec in want]
    if z >= 0:  # dropped and undropped pairs
        assert any(f & bc.ZDROPPED for f in flags) and any(not f & bc.ZDROPPED for f in flags), flags
        assert any(rec["lastDiag"] < len(r) + len(q) for (r, q), (_, _, rec) in zip(texts, want))
    else:
        assert not any(f & bc.ZDROPPED for f in flags)
    if e >= 0:  # end-to-end and clipped choices
        assert any(f & bc.REACHED_END for f in flags) and any(not f & bc.REACHED_END for f in flags), flags
    else:
        assert not any(f & bc.REACHED_END for f in flags)
    sb = from_strings(texts)
    got, _ = _long(gpu, BAXT, sb, band, w=w, table=table, z=z, e=e)
    _same(got, _direction(gpu, BAXT, sb, band, w=w, table=table, z=z, e=e), ("direction batch", with_table, z, e))
    _against_oracle(got, want, ("extension", with_table, z, e))


def test_extension_mode_across_band_classes(gpu, orc):
    """the drop test and the row-m pick-up at every cells-per-lane class, both parities"""
    texts = bc.extension_pairs(seed=6, count=12)
    sb = from_strings(texts)
    for band in (63, 64, 128, 129, 256, 300):
        want = orc.expect_all(BAXT, texts, band, zdrop=40, end_bonus=10)
        got, _ = _long(gpu, BAXT, sb, band, z=40, e=10)
        _against_oracle(got, want, ("classes", band))
        got, _ = _long(gpu, BAXT, sb, band, z=-1, e=10)
        _against_oracle(got, orc.expect_all(BAXT, texts, band, zdrop=-1, end_bonus=10), ("classes, bonus", band))


# ---------------------------------------------------------------------------------------- 4. reversed pairs

@pytest.mark.parametrize("algo,z", [(BANW, -1), (BAXT, 40)], ids=["BANW", "BAXT_zdrop"])
def test_reversed(gpu, orc, algo, z):
    texts = [t for t in bc.extension_pairs(seed=8, count=20) if algo != BANW or abs(len(t[0]) - len(t[1])) < 100]
    sb = from_strings(texts)
    mask = (np.arange(len(texts)) % 2).astype(np.uint8)
    got, _ = _long(gpu, algo, sb, 100, z=z, mask=mask)
    _same(got, _direction(gpu, algo, sb, 100, z=z, mask=mask), (NAME[algo], "reversed"))
    flipped = [(r[::-1], q[::-1]) if mask[p] else (r, q) for p, (r, q) in enumerate(texts)]  # the results stay in the reversed frame
    _against_oracle(got, orc.expect_all(algo, flipped, 100, zdrop=z), (NAME[algo], "reversed, oracle"))
    with gpu.Batch(algo, sb.sequences, sb.pairs, *W, band=100, flags=gpu.KEEP_BAND_DIRECTIONS | gpu.LONG_SCORES) as b:
        _apply(b, algo, None, z, -1)
        b.fill()
        forward = _results(b, False)
        b.set_reversed(mask)
        assert _status(gpu, b.results) == NOT_FILLED
        assert b.describe()["reversed"] == int(mask.sum())
        b.fill()
        assert _results(b, False)["scores"] == got["scores"]
        b.set_reversed(None)
        b.fill()
        _same(_results(b, False), forward, "mask cleared")


# ---------------------------------------------------------------------------------------- 5. the int16 twin

def _twin_pairs(algo):
    rng = np.random.default_rng(50 + algo)
    texts = []
    for k in range(32):
        m = int(rng.integers(300, 601))
        n = min(max(m + int(rng.integers(-99, 100)), 300), 600)
        texts.append(bc.related(rng, m, n) if k % 5 else bc.unrelated(rng, m, n))
    return texts + [(b"", b"ACGT"), (b"ACG", b""), (b"", b"")]


@pytest.mark.parametrize("algo", ALGOS, ids=[NAME[a] for a in ALGOS])
def test_equals_the_int16_score_only_batch(gpu, algo):
    texts = [t for t in _twin_pairs(algo) if algo != BANW or abs(len(t[0]) - len(t[1])) < 128]
    sb = from_strings(texts)
    got, _ = _long(gpu, algo, sb, 128)
    with gpu.Batch(algo, sb.sequences, sb.pairs, *bc.weights(algo), band=128, flags=gpu.SCORE_ONLY) as b:  # (a refusal raises: every pair is admitted)
        d = b.describe()
        assert d["store"] == 0 and d["kernel"] in ("k_banded_fill", "k_basw_fill", "k_banw_fill", "k_baxt_fill"), d
        b.fill()
        _same(got, _results(b, False), (NAME[algo], "int16 DPX_SCORE_ONLY"))
    # dpx_align_batch takes no flags: it stays the int16 one-shot, and agrees on these pairs
    s, r, c = (np.empty(len(texts), np.int32) for _ in range(3))
    prm = gpu.Params(algo, *bc.weights(algo), 128)
    pairs = np.ascontiguousarray(sb.pairs)
    rc = gpu.load().dpx_align_batch(C.byref(prm), sb.sequences.ctypes.data, sb.sequences.size, pairs.ctypes.data, len(pairs), s.ctypes.data,
                                    r.ctypes.data, c.ctypes.data, None, None, None)
    assert rc == 0
    assert (s.tolist(), list(zip(r.tolist(), c.tolist()))) == (got["scores"], got["ends"])


# ---------------------------------------------------------------------------------------- 6. pairs the int16 batch refuses

@pytest.mark.parametrize("algo", ALGOS, ids=[NAME[a] for a in ALGOS])
@pytest.mark.parametrize("which", [0, 1], ids=["33000_band64", "20000x20300_band256"])
def test_long_pairs_the_int16_batch_refuses(gpu, orc, algo, which):
    ref, qry, band = bc.long_pairs()[which]
    if algo == BANW and abs(len(ref) - len(qry)) >= band:
        ref = ref[:len(qry) + band - 1]  # BANW's admission rule |m - n| < B: the same pair, its reference cut to |m - n| = B - 1
    sb = from_strings([(ref, qry)])
    assert _status(gpu, gpu.Batch, algo, sb.sequences, sb.pairs, *bc.weights(algo), band=band, flags=gpu.SCORE_ONLY) == RANGE
    want = orc.expect_all(algo, [(ref, qry)], band, w=bc.weights(algo))
    assert want[0][0] > 32767
    got, d = _long(gpu, algo, sb, band)
    assert d["waves_per_workgroup"] == 1  # four waves' strings do not fit a workgroup's LDS
    _against_oracle(got, want, (NAME[algo], "long", which))


@pytest.mark.parametrize("algo", ALGOS, ids=[NAME[a] for a in ALGOS])
def test_a_700_base_pair_under_entries_100_to_127(gpu, orc, algo):
    table = bc.high_table()
    assert table[0].min() == 100 and table[0].max() == 127
    rng = np.random.default_rng(9)
    texts = [bc.related(rng, 700, 700), bc.related(rng, 700, 690)]
    sb = from_strings(texts)
    w = (2, -3) + TABLE_GAPS[2:]
    with gpu.Batch(algo, sb.sequences, sb.pairs, *bc.weights(algo, w), band=64, flags=gpu.SCORE_ONLY) as b:
        if bc.is_local(algo):  # (the int16 BSW / BASW batches have no table setter at all)
            assert _status(gpu, b.set_substitution, *table) == UNSUPPORTED
        else:
            assert _status(gpu, b.set_substitution, *table) == RANGE
    got, _ = _long(gpu, algo, sb, 64, w=w, table=table)
    want = orc.expect_all(algo, texts, 64, w=bc.weights(algo, w), table=table)
    assert min(s for s, _, _ in want) > 32767
    _against_oracle(got, want, (NAME[algo], "high table"))


# ---------------------------------------------------------------------------------------- 7. surface

def test_create_statuses(gpu):
    sb = from_strings([bc.related(np.random.default_rng(1), 200, 210)] * 2)
    L, G, S = gpu.KEEP_LOCAL_BAND_DIRECTIONS, gpu.KEEP_BAND_DIRECTIONS, gpu.LONG_SCORES
    create = lambda algo, flags, band=16: _status(gpu, gpu.Batch, algo, sb.sequences, sb.pairs, *bc.weights(algo), band=band, flags=flags)
    for algo in ALGOS:
        storage = _storage(gpu, algo)
        assert create(algo, S) == INVALID and create(algo, S | G | L) == INVALID and create(algo, S | storage | gpu.SCORE_ONLY) == INVALID, NAME[algo]
        assert create(algo, S | storage | gpu.KEEP_DIRECTIONS) == UNSUPPORTED and create(algo, S | (G | L) ^ storage) == UNSUPPORTED, NAME[algo]
        assert create(algo, S | storage, band=513) == UNSUPPORTED and create(algo, S | storage, band=512) == 0, NAME[algo]
        assert create(algo, storage | gpu.SCORE_ONLY) == INVALID  # pinned, and stays
    assert create(BANW, S | G | gpu.TWO_PIECE_GAPS) == UNSUPPORTED and create(BAXT, S | G | gpu.TWO_PIECE_GAPS) == UNSUPPORTED
    assert create(BASW, S | L | gpu.LOCAL_TWO_PIECE_GAPS) == UNSUPPORTED
    for algo in (0, 1, 2, 4, 6):
        assert create(algo, S | G, band=0) == UNSUPPORTED and create(algo, S | L, band=0) == UNSUPPORTED and create(algo, S, band=0) == INVALID, algo
    assert create(BANW, S | G, band=10) == UNSUPPORTED  # |m - n| = 10 >= B: BANW's admission rule


@pytest.mark.parametrize("algo", ALGOS, ids=[NAME[a] for a in ALGOS])
def test_no_matrix_answers_and_refusing_setters(gpu, orc, algo):
    rng = np.random.default_rng(21)
    texts = [bc.related(rng, 200, 210), bc.related(rng, 150, 140)]
    sb = from_strings(texts)
    table = bc.ACGTN_TABLE
    want = orc.expect_all(algo, texts, 16, w=bc.weights(algo))
    with gpu.Batch(algo, sb.sequences, sb.pairs, *bc.weights(algo), band=16, flags=_storage(gpu, algo) | gpu.LONG_SCORES | gpu.TUNE_PLACEMENT) as b:
        _ran_score_only(gpu, b, algo, 16)  # (DPX_TUNE_PLACEMENT is ignored: there is no pool to shop for)
        b.fill()
        first = _results(b, False)
        _against_oracle(first, want, NAME[algo])
        six = [_status(gpu, b.matrix, 0), _status(gpu, b.directions, 0), _status(gpu, b.traceback, 0), _status(gpu, b.output_begin, 0),
               _status(gpu, b.cigars_begin), _status(gpu, b.diffs_begin)]
        assert six == [NO_MATRIX] * 6, six
        assert _status(gpu, b.extensions) == UNSUPPORTED  # the fill ran no scan
        before = b.describe()
        refusing = [lambda: b.set_substitution(*table), lambda: b.set_extension(100, -1), lambda: b.set_extension_table(100, -1, *table),
                    lambda: b.set_second_gap(-24, -1), lambda: b.set_direction_table(*table), lambda: b.set_score_table(*table)]
        if bc.is_local(algo):
            refusing += [lambda: b.set_direction_scoring(-1, -1, *table), lambda: b.set_direction_scoring(100, -1), lambda: b.set_reversed(np.ones(2, np.uint8))]
        else:
            refusing += [lambda: b.set_local_direction_table(*table)]
            if algo == BANW:
                refusing += [lambda: b.set_direction_scoring(100, -1), lambda: b.set_direction_scoring(-1, 5, *table)]
        statuses = [_status(gpu, call) for call in refusing]
        assert all(s == UNSUPPORTED for s in statuses), statuses
        assert b.describe() == before  # the batch is left as it was ...
        _same(_results(b, False), first, "after the refused settings")  # ... its fill still valid
        b.fill()
        _same(_results(b, False), first, "repeated fill")


def test_plumbing_caller_stream_packed2_repeated_and_timed_fills(gpu, orc):
    hip = C.CDLL("libamdhip64.so")
    handle = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(handle), 1) == 0 and handle.value  # hipStreamNonBlocking
    rng = np.random.default_rng(80)
    texts = [bc.related(rng, 300, 310), bc.related(rng, 120, 100), (b"", b"ACGT"), (b"ACGT", b"")]
    sb = from_strings(texts)
    band = 140
    for algo in ALGOS:
        want = orc.expect_all(algo, texts, band, w=bc.weights(algo))
        got, _ = _long(gpu, algo, sb, band, fill=lambda b: b.fill(handle.value))  # no synchronisation between create and this fill
        _against_oracle(got, want, (NAME[algo], "caller's stream"))
        pk, al = gpu.pack2(sb.sequences, sb.pairs)
        got, d = _long(gpu, algo, sb, band, packed2=(pk, al, sb.sequences.size))
        assert d["seq_input"] == "packed2"
        _against_oracle(got, want, (NAME[algo], "packed2"))

        def timed(b):
            b.fill()
            first = b.results()
            b.fill()
            assert b.fill_timed(3) > 0.0
            assert all(np.array_equal(x, y) for x, y in zip(first, b.results()))
        got, _ = _long(gpu, algo, sb, band, fill=timed, extra_flags=gpu.TIME_FILLS, device=0)  # dpx_batch_create_on
        _against_oracle(got, want, (NAME[algo], "timed"))
        dev = None
        with gpu.Batch(algo, sb.sequences, sb.pairs, *bc.weights(algo), band=band, flags=_storage(gpu, algo) | gpu.LONG_SCORES) as b:
            b.fill()
            b.sync()
            dev = b.device_results()
            assert all(dev) and len(set(dev)) == 3
    assert hip.hipStreamDestroy(handle) == 0
