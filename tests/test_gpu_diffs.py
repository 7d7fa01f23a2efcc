"""dpx_batch_diffs_begin / _end on the device: the MD and cs string of every pair equals tests/diff_ref.py applied to the lines the same
batch returns through dpx_batch_traceback (the existing suites pin those per algorithm), for every algorithm and storage mode; every
adjacency of two classes, number widths up to six digits, alignment lengths and breakers around the 256-column trips and all four
skews, the scan across tiles with empty alignments mixed in, arbitrary bytes, reversed pairs, and the order / state rules."""
import ctypes as C
import itertools

import numpy as np
import pytest

import diff_ref as R
from dpx_gpu_genomics_project_amd.synth import from_strings

pytestmark = pytest.mark.gpu
LIN = (3, -1, -2)
AFF = (3, -1, -3, -1)
INVALID, NOT_FILLED, NO_MATRIX = -1, -6, -7
MD, CS = 1, 2
BOTH = MD | CS
ACGT = np.frombuffer(b"ACGT", np.uint8)
ALGOS = {"LNW": (0, LIN, 0), "LSW": (1, LIN, 0), "ANW": (2, AFF, 0), "BSW": (3, LIN, 16), "ASW": (4, AFF, 0), "BASW": (5, AFF, 16),
         "ASG": (6, AFF, 0), "BANW": (7, AFF, 16), "BAXT": (10, AFF, 16)}


def _batch(gpu, algo, sb, flags=0, **kw):
    code, w, band = ALGOS[algo]
    return gpu.Batch(code, sb.sequences, sb.pairs, *w, band=kw.pop("band", band), flags=flags, **kw)


def _diffs(b, kinds=BOTH):
    """{kind: [bytes per pair]}; the offsets are checked on the way"""
    b.diffs_begin(kinds)
    out = {}
    for kind in (MD, CS):
        if kinds & kind:
            raw, offs = b.diffs_end(kind)
            assert raw.dtype == np.uint8 and offs.dtype == np.uint64 and len(offs) == b.num_pairs + 1
            assert int(offs[0]) == 0 and int(offs[-1]) == len(raw) and np.all(np.diff(offs.astype(np.int64)) >= 0)
            data = raw.tobytes()
            out[kind] = [data[int(offs[p]):int(offs[p + 1])] for p in range(b.num_pairs)]
            assert out[kind] == b.diff_strings(kind)
    return out


def _lines(b, p):
    return tuple(x.encode("latin-1") for x in b.traceback(p))


def _check(b, what="", pairs=None):
    """`b` is filled.  The diff path runs first, so it is the one that walks; the lines come from dpx_batch_traceback afterwards."""
    got = _diffs(b)
    picks = range(b.num_pairs) if pairs is None else pairs
    lines = {p: _lines(b, p) for p in picks}
    for kind in (MD, CS):
        for p in picks:
            want = R.KINDS[kind](lines[p])
            assert got[kind][p] == want, (what, kind, p, got[kind][p][:200], want[:200])
    return got, lines


def _mutated(rng, ref, subs=0.08, indels=0.04):
    out = bytearray()
    for c in ref:
        r = rng.random()
        if r < indels / 2:
            continue
        if r < indels:
            out.append(int(ACGT[rng.integers(0, 4)]))
        out.append(c if rng.random() >= subs else int(ACGT[rng.integers(0, 4)]))
    return bytes(out)


def _ragged(rng, count=48, lo=30, hi=150):
    """related pairs of lo..hi bases whose lengths differ by less than 16 (BANW admits the batch)"""
    texts = []
    while len(texts) < count:
        ref = ACGT[rng.integers(0, 4, int(rng.integers(lo + 8, hi + 1)))].tobytes()
        qry = _mutated(rng, ref)[:hi]
        if abs(len(ref) - len(qry)) >= 16:
            k = min(len(ref), len(qry))
            ref, qry = ref[:k], qry[:k]
        if min(len(ref), len(qry)) >= lo:
            texts.append((ref, qry))
    return from_strings(texts)


def _table(gpu):
    scores = np.full((5, 5), -2, np.int8)
    np.fill_diagonal(scores, 3)
    scores[4, :] = scores[:, 4] = -1
    return scores, gpu.code_table(b"ACGTN")


# ------------------------------------------------------------------------------------------------------------------ 6. every route

ROUTES = [(algo, "matrices") for algo in ALGOS] + [(algo, "directions") for algo in ("LNW", "LSW", "ANW", "ASW", "ASG")] + \
         [(algo, mode) for algo in ("BANW", "BAXT") for mode in ("band_directions", "two_piece")] + \
         [("BSW", "local_band_directions"), ("BASW", "local_band_directions"), ("BAXT", "extension_table")]


@pytest.mark.parametrize("algo,mode", ROUTES)
def test_every_route(gpu, algo, mode):
    sb = _ragged(np.random.default_rng(600 + ALGOS[algo][0]))
    assert sb.num_pairs == 48 and sb.pairs["querySize"].min() >= 30 and sb.pairs["referenceSize"].max() <= 150
    flags = {"matrices": gpu.KEEP_MATRICES, "directions": gpu.KEEP_DIRECTIONS, "band_directions": gpu.KEEP_BAND_DIRECTIONS,
             "two_piece": gpu.KEEP_BAND_DIRECTIONS | gpu.TWO_PIECE_GAPS, "local_band_directions": gpu.KEEP_LOCAL_BAND_DIRECTIONS,
             "extension_table": gpu.KEEP_MATRICES}[mode]
    if mode == "two_piece":  # a short steep piece and a long flat one
        b = gpu.Batch(ALGOS[algo][0], sb.sequences, sb.pairs, 3, -1, -4, -2, band=ALGOS[algo][2], flags=flags)
    else:
        b = _batch(gpu, algo, sb, flags=flags)
    with b:
        if mode == "two_piece":
            b.set_second_gap(-24, -1)
        if mode == "extension_table":
            b.set_extension_table(100, 5, *_table(gpu))
        b.fill()
        got, lines = _check(b, what=(algo, mode))
    cls = "".join(R.classes(lines[p]) for p in lines)
    assert all(c in cls for c in "=XDI"), (algo, mode)  # (nothing compares empty)
    assert len(set(got[MD])) > 40 and len(set(got[CS])) > 40


# ------------------------------------------------------------------------------------------------------------------ 7. adjacencies

def _adjacency_pairs():
    rng = np.random.default_rng(7)
    left = ACGT[rng.integers(0, 4, 40)].tobytes() + b"G"
    right = b"T" + ACGT[rng.integers(0, 4, 40)].tobytes()
    crafted = [(left + right, left + b"_N_" + right),              # an inserted _N_ reads as D,I,D
               (left + right, left + b"N_N" + right),              # ... and N_N as I,D,I
               (left + b"A" + right, left + b"C" + right),         # =X X=
               (left + b"AA" + right, left + b"CC" + right),       # XX
               (left + b"A" + right, left + b"CNN" + right),       # a mismatch next to an insertion: XI or IX by the tie rule
               (left + b"ACCC" + right, left + b"G" + right),      # a mismatch next to a deletion: XD or DX
               (left + b"A" + right, left + b"C_" + right),        # ... and next to an inserted _, which reads as D
               (left + b"A" + right, left + b"_C" + right)]
    # every pair as it is and reversed on the device (the flagged pair's ties fall at the other end), and the mirrored strings likewise
    texts = [t for ref, qry in crafted for t in ((ref, qry), (ref, qry), (ref[::-1], qry[::-1]), (ref[::-1], qry[::-1]))]
    return from_strings(texts), (np.arange(len(texts)) % 2).astype(np.uint8)


def test_adjacencies(gpu):
    sb, mask = _adjacency_pairs()
    assert sb.num_pairs <= 64 and max(sb.pairs["querySize"].max(), sb.pairs["referenceSize"].max()) < 200
    with _batch(gpu, "BANW", sb) as b:
        b.set_reversed(mask)
        b.fill()
        got, lines = _check(b, what="adjacencies")
    cls = [R.classes(lines[p]) for p in range(sb.num_pairs)]
    for a, c in itertools.permutations("=XDI", 2):
        assert any(a + c in s for s in cls), (a + c, cls)
    assert any("DID" in s for s in cls)
    assert any(b"0^" in t for t in got[MD]) and any(t.count(b"^") >= 2 for t in got[MD])


# ---------------------------------------------------------------------------------------------------------------- 8. number widths

def _one_substitution(rng, front, back):
    """identical random sequences of front + 1 + back bases with the base at `front` substituted"""
    ref = ACGT[rng.integers(0, 4, front + 1 + back)].copy()
    qry = ref.copy()
    qry[front] = ACGT[(int(np.where(ACGT == ref[front])[0][0]) + 1) % 4]
    return ref.tobytes(), qry.tobytes()


def test_number_widths_up_to_five_digits(gpu):
    rng = np.random.default_rng(8)
    runs = (9, 10, 99, 100, 999, 1000, 9999, 10000)
    texts = [_one_substitution(rng, r, r) for r in runs]
    with _batch(gpu, "LNW", from_strings(texts), flags=gpu.KEEP_DIRECTIONS) as b:
        b.fill()
        got, _ = _check(b, what="widths")
    for p, r in enumerate(runs):
        ref, qry = texts[p]
        assert got[MD][p] == b"%d%c%d" % (r, ref[r], r), (r, got[MD][p])
        assert got[CS][p] == b":%d*%c%c:%d" % (r, ref[r] + 32, qry[r] + 32, r), (r, got[CS][p])


def test_numbers_carried_across_three_hundred_trips(gpu):
    """The longest match runs a batch can produce in test time: BANW band-direction pairs of 80 002 bases at band 16.  Runs of 99 999 and
    100 000 (six digits) were asked for on a pair of about 100 001 bases, but a band-direction fill stages both strings of a pair in one
    workgroup's LDS (160 KiB), so dpx_batch_create refuses pairs beyond m + n of about 163 000 with DPX_ERR_UNSUPPORTED, and a
    full-matrix direction batch of 100 001^2 cells is one wave's work for many seconds.  So no test reaches six digits on the device;
    the digit count is the ten-step compare chain of dpx_diff_kernels.hip and the digit loop does not depend on the width."""
    rng = np.random.default_rng(9)
    shapes = [(80000, 1), (1, 80000), (79999, 2), (2, 79999)]
    texts = [_one_substitution(rng, f, k) for f, k in shapes]
    with _batch(gpu, "BANW", from_strings(texts), flags=gpu.KEEP_BAND_DIRECTIONS, band=16) as b:
        b.fill()
        got, _ = _check(b, what="long runs")
    for p, (f, k) in enumerate(shapes):
        ref, qry = texts[p]
        assert got[MD][p] == b"%d%c%d" % (f, ref[f], k), (f, k, got[MD][p])
        assert got[CS][p] == b":%d*%c%c:%d" % (f, ref[f] + 32, qry[f] + 32, k), (f, k, got[CS][p])


# ------------------------------------------------------------------------------------------------------ 9. trip and skew boundaries

LENGTHS = list(range(1, 13)) + list(range(252, 261)) + list(range(508, 517))


def _skew(sb, p, lines):
    cap = (int(sb.pairs["querySize"][p]) + int(sb.pairs["referenceSize"][p]) + 1 + 3) & ~3
    return (cap - len(lines[1])) & 3


def test_alignment_lengths_around_the_trips_under_every_skew(gpu):
    rng = np.random.default_rng(10)
    texts = [_one_substitution(rng, n // 2, n - 1 - n // 2) for n in LENGTHS]
    texts += [(r, q[:-1]) for r, q in texts] + [(r[:-1], q + b"A") for r, q in texts if len(r) > 1]  # other capacities: other skews
    sb = from_strings(texts)
    with _batch(gpu, "ANW", sb) as b:
        b.fill()
        got, lines = _check(b, what="lengths")
    seen = {(len(lines[p][1]), _skew(sb, p, lines[p])) for p in lines}
    assert {n for n, _ in seen} >= set(LENGTHS) and {s for _, s in seen} == {0, 1, 2, 3}


def test_breakers_and_runs_on_the_trip_boundaries(gpu):
    rng = np.random.default_rng(11)
    texts = []
    for total in (600, 601, 602, 603):  # four capacities: all four skews
        for col in (0, 255, 256, 257, 511, 512, total - 1):
            texts.append(_one_substitution(rng, col, total - 1 - col))
        base = ACGT[rng.integers(0, 4, total)].tobytes()
        extra = ACGT[rng.integers(0, 4, 12)].tobytes()
        texts.append((base[:250] + extra + base[250:], base))   # a deletion run across the first trip boundary
        texts.append((base, base[:250] + extra + base[250:]))   # ... an insertion run
        texts.append((base[:506] + extra + base[506:], base))   # ... and across the second
        texts.append((base + base[:200], base + base[:200]))    # a match run open across three trips
        texts.append((base, b""))                               # a deletion run open across three trips
        texts.append((b"", base))                               # an insertion run
    sb = from_strings(texts)
    with _batch(gpu, "ANW", sb) as b:
        b.fill()
        got, lines = _check(b, what="boundaries")
    assert {_skew(sb, p, lines[p]) for p in lines} == {0, 1, 2, 3}
    cls = [R.classes(lines[p]) for p in range(sb.num_pairs)]
    for col in (0, 255, 256, 257, 511, 512):
        assert any(len(s) > col and s[col] == "X" for s in cls), col
    assert any(s.endswith("X") for s in cls)
    assert any("D" * 12 in s and s.index("D") < 256 <= s.rindex("D") for s in cls)
    assert any("D" * 12 in s and s.index("D") < 512 <= s.rindex("D") for s in cls)
    assert any(s == "=" * len(s) and len(s) >= 800 for s in cls) and any(s == "D" * len(s) and len(s) >= 600 for s in cls)
    assert any(m == b"%d" % len(s) for m, s in zip(got[MD], cls) if len(s) >= 800)


# --------------------------------------------------------------------------------------------------------------- 10. scan across tiles

def _tiny_pairs(count=5000):
    """lengths 0..12; a third of the pairs share no base, so their local alignment is empty and their extension ends at (0, 0)"""
    rng = np.random.default_rng(5000)
    texts = []
    for p in range(count):
        n, m = int(rng.integers(0, 13)), int(rng.integers(0, 13))
        if p % 3 == 0:
            texts.append((b"AC"[int(rng.integers(0, 2))::2] * n, b"GT"[int(rng.integers(0, 2))::2] * m))
        else:
            texts.append((ACGT[rng.integers(0, 4, n)].tobytes(), ACGT[rng.integers(0, 4, m)].tobytes()))
    return from_strings(texts)


@pytest.mark.parametrize("algo", ["LSW", "BAXT"])
def test_scan_across_tiles(gpu, algo):
    sb = _tiny_pairs()
    with _batch(gpu, algo, sb) as b:
        b.fill()
        got, lines = _check(b, what="5000 tiny pairs", pairs=range(0, sb.num_pairs, 2))  # (the offsets are checked for all)
        empty = [p for p in lines if len(lines[p][1]) == 0]
    assert len(empty) >= 800 and len(lines) - len(empty) >= 300
    assert all(got[MD][p] == b"0" and got[CS][p] == b"" for p in empty)
    assert sum(len(t) for t in got[MD]) > 5000 and sum(len(t) > 0 for t in got[CS]) > 500


# ------------------------------------------------------------------------------------------------------------------ 11. arbitrary bytes

def test_arbitrary_bytes(gpu):
    rng = np.random.default_rng(256)
    texts = []
    for _ in range(32):
        ref = rng.integers(0, 256, int(rng.integers(40, 300))).astype(np.uint8)
        qry = bytearray()
        for c in ref.tolist():
            r = rng.random()
            if r < 0.03:
                continue
            if r < 0.06:
                qry.append(int(rng.integers(0, 256)))
            qry.append(c if rng.random() >= 0.1 else int(rng.integers(0, 256)))
        texts.append((ref.tobytes(), bytes(qry)))
    with _batch(gpu, "LNW", from_strings(texts)) as b:
        b.fill()
        got, lines = _check(b, what="256 symbols")
    emitted = set(b"".join(got[MD]))
    assert 0 in emitted and ord("^") in emitted and len(emitted) > 200   # NUL, and more than digits and letters
    assert any(R.lc(c) != c for p in lines for c in lines[p][0]) and set(b"".join(got[CS])) & set(range(0x41, 0x5B)) == set()


# ------------------------------------------------------------------------------------------------------------------ 12. reversed pairs

@pytest.mark.parametrize("algo", ["BANW", "BAXT"])
def test_reversed_pairs(gpu, algo):
    sb = _ragged(np.random.default_rng(1200))
    mask = (np.arange(sb.num_pairs) % 2).astype(np.uint8)
    with _batch(gpu, algo, sb) as b:
        b.fill()
        plain, _ = _check(b, what=(algo, "forward"))
        b.set_reversed(mask)
        b.fill()
        got, lines = _check(b, what=(algo, "half reversed"))
        b.cigars_begin(gpu.CIGAR_EXTENDED)
        recs, _ = b.cigars_end()
    assert any(got[MD][p] != plain[MD][p] for p in range(1, sb.num_pairs, 2))
    for p in range(sb.num_pairs):
        cls = R.classes(lines[p])
        nm = int(recs["mismatches"][p]) + int(recs["insertions"][p]) + int(recs["deletions"][p])
        assert nm == len(cls) - cls.count("="), p


# ------------------------------------------------------------------------------------------------------------------ 13. order and state

def test_text_cigars_and_diffs_in_every_order(gpu):
    sb = _ragged(np.random.default_rng(1300), count=24)
    with _batch(gpu, "ANW", sb) as b:
        b.fill()
        want, _ = _check(b)
        b.fill()
        b.output_begin(3)
        text = b.output_end()[0]
        b.fill()
        b.cigars_begin(gpu.CIGAR_EXTENDED)
        recs, ops = b.cigars_end()
        begin = {"text": lambda: b.output_begin(3), "cigars": lambda: b.cigars_begin(gpu.CIGAR_EXTENDED), "diffs": lambda: b.diffs_begin(BOTH)}
        for order in itertools.permutations(("text", "cigars", "diffs")):
            b.fill()
            for step in order:  # all three in flight behind one fill, then collected
                begin[step]()
            got_recs, got_ops = b.cigars_end()
            assert {k: b.diff_strings(k) for k in (MD, CS)} == want, order
            assert b.output_end()[0] == text and got_recs.tobytes() == recs.tobytes() and np.array_equal(got_ops, ops), order


def test_kinds_alone_and_together_and_end_twice(gpu):
    sb = _ragged(np.random.default_rng(1301), count=24)
    with _batch(gpu, "LSW", sb) as b:
        b.fill()
        want = _diffs(b)
        for kind in (MD, CS):
            b.fill()
            b.diffs_begin(kind)
            assert b.diff_strings(kind) == want[kind]
            assert b.diff_strings(kind) == want[kind]  # _end again: the same contents
            with pytest.raises(gpu.DpxError) as e:
                b.diffs_end(BOTH ^ kind)  # the other kind was not begun since this fill
            assert e.value.status == NOT_FILLED
            b.diffs_begin(BOTH ^ kind)  # a later _begin of the other kind leaves this one's result alone
            assert b.diff_strings(BOTH ^ kind) == want[BOTH ^ kind] and b.diff_strings(kind) == want[kind]
    assert want[MD] != want[CS]


def test_state_and_errors(gpu):
    sb = _ragged(np.random.default_rng(1302), count=8)
    with _batch(gpu, "LNW", sb) as b:
        for call in (lambda: b.diffs_begin(BOTH), lambda: b.diffs_end(MD), lambda: b.diffs_end(CS)):
            with pytest.raises(gpu.DpxError) as e:
                call()
            assert e.value.status == NOT_FILLED
        b.fill()
        with pytest.raises(gpu.DpxError) as e:
            b.diffs_end(MD)  # no _begin yet
        assert e.value.status == NOT_FILLED
        for bad in (0, 4, 8, 0x10, 0x80000000, 5, 7):
            with pytest.raises(gpu.DpxError) as e:
                b.diffs_begin(bad)
            assert e.value.status == INVALID, bad
        for bad in (0, 3, 4, 0x80000001):
            with pytest.raises(gpu.DpxError) as e:
                b.diffs_end(bad)
            assert e.value.status == INVALID, bad
        first = _diffs(b)
        b.fill()
        for kind in (MD, CS):
            with pytest.raises(gpu.DpxError) as e:
                b.diffs_end(kind)  # the second fill invalidated them
            assert e.value.status == NOT_FILLED
        assert _diffs(b) == first
    lib = gpu.load()
    assert lib.dpx_batch_diffs_begin(None, MD) == INVALID and lib.dpx_batch_diffs_end(None, MD, None, None, None) == INVALID
    with _batch(gpu, "LNW", sb, flags=gpu.SCORE_ONLY) as b:
        b.fill()
        with pytest.raises(gpu.DpxError) as e:
            b.diffs_begin(MD)
        assert e.value.status == NO_MATRIX
    with _batch(gpu, "LSW", sb, num_pairs=0) as b:  # a batch without pairs
        b.fill()
        b.diffs_begin(BOTH)
        for kind in (MD, CS):
            raw, offs = b.diffs_end(kind)
            assert len(raw) == 0 and offs.tolist() == [0]


def test_the_text_ends_with_one_nul(gpu):
    sb = _ragged(np.random.default_rng(1303), count=8)
    lib = gpu.load()
    with _batch(gpu, "LNW", sb) as b:
        b.fill()
        b.diffs_begin(BOTH)
        for kind in (MD, CS):
            text, nbytes, offs = C.c_void_p(), C.c_size_t(0), C.POINTER(C.c_uint64)()
            assert lib.dpx_batch_diffs_end(b._h, kind, C.byref(text), C.byref(nbytes), C.byref(offs)) == 0
            assert nbytes.value == offs[sb.num_pairs] > 0 and C.string_at(text.value + nbytes.value, 1) == b"\0"
            assert lib.dpx_batch_diffs_end(b._h, kind, None, None, None) == 0  # every out pointer is optional


# ------------------------------------------------------------------------------------------------------------------ 14. recycled buffers

def test_recycled_buffers(gpu):
    """a large batch's strings, destroy, then a small batch's: the second batch takes the first one's parked buffers and its bytes
    depend on nothing left in them"""
    rng = np.random.default_rng(1400)
    big = _ragged(rng, count=400, lo=100, hi=150)
    small = _ragged(rng, count=10, lo=30, hi=40)
    with _batch(gpu, "ANW", small) as b:
        b.fill()
        want, _ = _check(b, what="small, fresh")
    for _ in range(2):
        with _batch(gpu, "ANW", big) as b:
            b.fill()
            _check(b, what="big", pairs=range(0, 400, 37))
        with _batch(gpu, "ANW", small) as b:
            b.fill()
            got, _ = _check(b, what="small, recycled")
            assert got == want


# ------------------------------------------------------------------------------------------------------------------ 15. caller's stream

def test_caller_stream(gpu):
    hip = C.CDLL("libamdhip64.so")
    handle = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(handle), 1) == 0 and handle.value   # hipStreamNonBlocking
    sb = _ragged(np.random.default_rng(1500), count=9)
    with _batch(gpu, "ANW", sb) as b:
        b.fill()
        want, _ = _check(b)
    for rep in range(4):
        with _batch(gpu, "ANW", sb) as b:
            b.fill(handle.value)  # no synchronisation between create, this fill and _begin
            kinds = (BOTH, MD, CS, BOTH)[rep]
            b.diffs_begin(kinds)
            assert all(b.diff_strings(k) == want[k] for k in (MD, CS) if kinds & k), rep
    assert hip.hipStreamDestroy(handle) == 0
