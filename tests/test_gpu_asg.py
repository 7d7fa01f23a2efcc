"""DPX_ALGO_ASG (affine-gap semi-global alignment) on the GPU against the CPU oracle tests/asg_oracle.c, bit-exact: every fill path,
every place the last query row can live in a wave, placed end cells (two equal maxima, column 0, negative and zero scores, empty
inputs), the lane-packed short-read batch, direction batches with both edge-row placements, range limits and the plumbing (packed2,
dpx_align_batch, weights of both signs, 256 symbols, a caller's stream).  Every case runs under the default wave walk and the lane walk."""
import ctypes as C
import zlib

import numpy as np
import pytest

import asg_ref
from dpx_gpu_genomics_project_amd.synth import from_strings

pytestmark = pytest.mark.gpu

ASG = 6
W = (3, -1, -3, -1)
INVALID, RANGE = -1, -4


@pytest.fixture(autouse=True, params=["wave-walk", "lane-walk"])
def walk(request, monkeypatch):
    """Every test of this file on both tracebacks: k_traceback_wave<3, false, ASG> (one wave per pair, the default up to 20 000 pairs)
    and, with DPX_TB_WALK=0, k_asg_traceback (one lane per pair)."""
    if request.param == "lane-walk":
        monkeypatch.setenv("DPX_TB_WALK", "0")
    return request.param


@pytest.fixture(scope="module")
def asg(tmp_path_factory):
    return asg_ref.build(tmp_path_factory.mktemp("asg_gpu"))


def _window_pair(rng, m, n, alphabet=4, base=65):
    """a query that is a mutated window of its reference"""
    ref = rng.integers(0, alphabet, n).astype(np.uint8) + base
    start = int(rng.integers(0, max(n - m, 0) + 1))
    q = ref[start:start + m].copy()
    q = np.concatenate([q, (rng.integers(0, alphabet, m - len(q)) + base).astype(np.uint8)])
    sub = rng.random(m) < 0.12
    q[sub] = (rng.integers(0, alphabet, int(sub.sum())) + base).astype(np.uint8)
    q = q[~(rng.random(m) < 0.03)]
    return ref.astype(np.uint8).tobytes(), q.astype(np.uint8).tobytes()


def _related(seed, count, mq, nr, empties=True):
    rng = np.random.default_rng(seed)
    texts = [_window_pair(rng, int(rng.integers(mq[0], mq[1] + 1)), int(rng.integers(nr[0], nr[1] + 1))) for _ in range(count)]
    if empties and count >= 3:
        texts[1] = (b"", texts[1][1])
        texts[2] = (texts[2][0], b"")
    return from_strings(texts)


_WANT = {}


def _want(asg, sb, w):
    """the oracle's results of a batch, computed once per (batch, weights) and shared by the walks and flags that need them"""
    key = (zlib.crc32(sb.sequences.tobytes()), zlib.crc32(sb.pairs.tobytes()), tuple(w))
    if key not in _WANT:
        _WANT[key] = [asg.align(sb.ref(p), sb.qry(p), *w) for p in range(sb.num_pairs)]
    return _WANT[key]


def _block(number, r):
    return b"%d | %d\n" % (number, r["score"]) + b"".join(x + b"\n" for x in r["lines"])


def _check(gpu, asg, sb, w=W, flags=None, matrices="sample", text=True, kernel="k_asg_fill", **kw):
    flags = gpu.KEEP_MATRICES if flags is None else flags
    dirs = bool(flags & gpu.KEEP_DIRECTIONS)
    want = _want(asg, sb, w)
    with gpu.Batch(ASG, sb.sequences, sb.pairs, *w, flags=flags, **kw) as b:
        d = b.describe()
        assert d["algo"] == "ASG" and d["kernel_algo"] == "ASG" and d["kernel"] == ("k_asg_dir" if dirs else kernel), d
        b.fill()
        scores, rows, cols = b.results()
        for p, r in enumerate(want):
            assert (scores[p], rows[p], cols[p]) == (r["score"], *r["end"]), (p, sb.ref(p), sb.qry(p))
        if flags & gpu.SCORE_ONLY:
            return d
        if matrices:
            picks = range(sb.num_pairs) if matrices == "all" else sorted({0, sb.num_pairs - 1} |
                                                                         set(np.random.default_rng(3).choice(sb.num_pairs, min(4, sb.num_pairs), replace=False).tolist()))
            for p in picks:
                if dirs:  # the reference's enums, borders included
                    for which, key in ((gpu.MAT_H, "dirH"), (gpu.MAT_I, "dirI"), (gpu.MAT_D, "dirD")):
                        assert np.array_equal(b.directions(p, which), want[p][key]), (p, key)
                    continue
                for which, key in ((gpu.MAT_H, "H"), (gpu.MAT_I, "I"), (gpu.MAT_D, "D")):
                    assert np.array_equal(b.matrix(p, which).astype(np.int32), want[p][key]), (p, key)
        if text:
            for p, r in enumerate(want):
                assert tuple(x.encode("latin-1") for x in b.traceback(p)) == r["lines"], p
            b.output_begin(5)
            out, offs = b.output_end()
            assert out == b"".join(_block(5 + p, r) for p, r in enumerate(want))
        return d


# ---------------------------------------------------------------------------------------------------------------- fill paths

@pytest.mark.parametrize("R,mq,nr", [("2", (60, 128), (50, 200)), ("4", (129, 256), (100, 300)), ("8", (257, 512), (200, 600)),   # single stripe
                                     ("2", (300, 700), (128, 400)),   # several stripes, rolling schedule (n >= 128)
                                     ("2", (300, 600), (20, 120)),    # several stripes, n < 128: striped schedule
                                     ("4", (300, 600), (20, 120)), ("8", (600, 1100), (128, 300))])
def test_fill_paths(gpu, asg, monkeypatch, R, mq, nr):
    monkeypatch.setenv("DPX_R", R)
    sb = _related(zlib.crc32(f"{R}{mq}{nr}".encode()), 12, mq, nr)
    d = _check(gpu, asg, sb)
    assert d["rows_per_lane"] == int(R)
    _check(gpu, asg, sb, flags=gpu.SCORE_ONLY)


@pytest.mark.parametrize("n", [60, 140])  # striped (n < 128) and rolling (n >= 128) schedules once there are several stripes
def test_where_the_last_row_lives(gpu, asg, monkeypatch, n):
    """R = 2: m = 64R and 64R + 1 (last register of lane 63 / first register of lane 0 of a new stripe), m = 1, (m-1) % R = 0 and R-1,
    the same around the second stripe's end"""
    monkeypatch.setenv("DPX_R", "2")
    rng = np.random.default_rng(n)
    texts = []
    for m in (1, 2, 3, 4, 127, 128, 129, 130, 255, 256, 257, 258):       # exact lengths: substitutions only
        ref = (rng.integers(0, 4, n) + 65).astype(np.uint8)
        q = np.resize(ref[n // 3:], m).copy()
        sub = rng.random(m) < 0.12
        q[sub] = (rng.integers(0, 4, int(sub.sum())) + 65).astype(np.uint8)
        texts.append((ref.tobytes(), q.tobytes()))
    sb = from_strings(texts)
    assert [len(sb.qry(p)) for p in range(sb.num_pairs)] == [1, 2, 3, 4, 127, 128, 129, 130, 255, 256, 257, 258]
    d = _check(gpu, asg, sb, matrices="all")
    assert d["rows_per_lane"] == 2
    _check(gpu, asg, sb, flags=gpu.SCORE_ONLY)


def test_last_row_lengths_exactly(gpu, asg, monkeypatch):
    """queries of EXACTLY 1, 2, 3, 128, 129 and 257 rows (no deletions applied), each against a reference that ends in the query"""
    monkeypatch.setenv("DPX_R", "2")
    rng = np.random.default_rng(77)
    texts = []
    for m in (1, 2, 3, 4, 127, 128, 129, 256, 257):
        q = (rng.integers(0, 4, m) + 65).astype(np.uint8).tobytes()
        texts.append(((rng.integers(0, 4, 150) + 65).astype(np.uint8).tobytes() + q, q))      # the best column is n: the last cell of row m
        texts.append((q + (rng.integers(0, 4, 33) + 65).astype(np.uint8).tobytes(), q))       # ... and column m, free tail
    sb = from_strings(texts)
    want = _want(asg, sb, W)
    assert [r["end"][0] for r in want] == [len(sb.qry(p)) for p in range(sb.num_pairs)]
    _check(gpu, asg, sb, matrices="all")


# -------------------------------------------------------------------------------------------------------------- placed cases

def test_placed_cases(gpu, asg, monkeypatch):
    monkeypatch.setenv("DPX_R", "2")
    core = b"GATTACAGATTACA"
    sb = from_strings([(core + b"GG" + core, core), (b"AG", b"AC"), (b"ACGT", b""), (b"", b"ACGT"), (b"", b"")])
    want = _want(asg, sb, W)
    assert want[0]["end"] == (14, 14) and want[0]["score"] == 42          # two equal maxima in row m: the first column wins
    _check(gpu, asg, sb, matrices="all")
    for w, score, end in (((1, -10, -3, -1), -3 + 4 * -1, (4, 0)), ((3, -1, -3, -1), -4, (4, 4))):
        one = from_strings([(b"0000", b"1111")])
        r = _want(asg, one, w)[0]
        assert (r["score"], r["end"]) == (score, end)
        if end == (4, 0):
            assert r["lines"] == (b"____", b"    ", b"1111")               # a column-0 winner prints m deletions
        _check(gpu, asg, one, w=w, matrices="all")
        _check(gpu, asg, one, w=w, flags=gpu.KEEP_DIRECTIONS, matrices="all")
    zero = from_strings([(b"AG", b"AC")])
    w = (3, -3, -3, -1)
    r = _want(asg, zero, w)[0]
    assert r["H"][2].tolist() == [-5, -1, 0] and r["end"] == (2, 2) and r["lines"] == (b"AG", b"*|", b"AC") and r["score"] == 0
    _check(gpu, asg, zero, w=w, matrices="all")                           # score 0 with a path: not LSW's empty block
    with gpu.Batch(ASG, zero.sequences, zero.pairs, *w) as b:
        b.fill()
        b.output_begin(0)
        assert b.output_end()[0] == b"0 | 0\nAG\n*|\nAC\n"
    empties = from_strings([(b"ACGT", b""), (b"", b"ACGT"), (b"", b"")])
    we = _want(asg, empties, W)
    assert [(r["score"], r["end"]) for r in we] == [(0, (0, 0)), (-3 + 4 * -1, (4, 0)), (0, (0, 0))]
    assert we[0]["lines"] == (b"", b"", b"") and we[1]["lines"] == (b"____", b"    ", b"ACGT")
    _check(gpu, asg, empties, matrices="all")
    _check(gpu, asg, empties, flags=gpu.KEEP_DIRECTIONS, matrices="all")
    _check(gpu, asg, empties, flags=gpu.SCORE_ONLY)


# --------------------------------------------------------------------------------------------------------------- short reads

def test_short_reads_batch(gpu, asg):
    """a short-read batch runs lane-packed on k_asg_lanes (several pairs per wave)"""
    rng = np.random.default_rng(9)
    texts = []
    for k in range(3000):
        m = int(rng.integers(80, 131))
        if k < 30:
            m = (80, 81, 87, 88, 89, 95, 96, 97, 103, 128, 129, 127)[k % 12]      # m % 8 in {0, 1, 7}
        ref = (rng.integers(0, 4, int(rng.integers(100, 161))) + 65).astype(np.uint8)
        start = int(rng.integers(0, max(len(ref) - m, 0) + 1))
        q = ref[start:start + m].copy()
        q = np.concatenate([q, (rng.integers(0, 4, m - len(q)) + 65).astype(np.uint8)])
        sub = rng.random(m) < 0.1
        q[sub] = (rng.integers(0, 4, int(sub.sum())) + 65).astype(np.uint8)
        texts.append((ref.tobytes(), q.tobytes()))
    sb = from_strings(texts)
    assert {len(sb.qry(p)) % 8 for p in range(30)} >= {0, 1, 7}
    d = _check(gpu, asg, sb, matrices=None, text=False, kernel="k_asg_lanes")
    assert d["lane_pairs"] > 0
    want = _want(asg, sb, W)
    with gpu.Batch(ASG, sb.sequences, sb.pairs, *W) as b:
        b.fill()
        b.output_begin(0)
        out, _ = b.output_end()
        for p in (0, 1, 2, 29, 2999):
            for which, key in ((gpu.MAT_H, "H"), (gpu.MAT_I, "I"), (gpu.MAT_D, "D")):
                assert np.array_equal(b.matrix(p, which).astype(np.int32), want[p][key]), (p, key)
    blocks = out.split(b"\n")
    for p in rng.choice(sb.num_pairs, 40, replace=False):
        assert b"\n".join(blocks[4 * p:4 * p + 4]) + b"\n" == _block(int(p), want[int(p)]), p
    _check(gpu, asg, sb, flags=gpu.SCORE_ONLY, kernel="k_asg_lanes")


def test_lanes_forced_with_placed_cases(gpu, asg, monkeypatch):
    """DPX_LANES=1 on a small batch: column-0 winners, empty sequences and the row lengths around a lane's 8 rows in one wave's slots"""
    monkeypatch.setenv("DPX_LANES", "1")
    core = b"GATTACAGATTACA"
    texts = [(core + b"GG" + core, core), (b"AG", b"AC"), (b"ACGT", b""), (b"", b"ACGT"), (b"", b""), (b"0000", b"1111"), (b"A", b"AA")]
    rng = np.random.default_rng(5)
    texts += [_window_pair(rng, m, 90) for m in (1, 7, 8, 9, 15, 16, 17, 63, 64, 65)]
    sb = from_strings(texts)
    _check(gpu, asg, sb, matrices="all", kernel="k_asg_lanes")
    _check(gpu, asg, sb, w=(1, -10, -3, -1), matrices="all", kernel="k_asg_lanes")
    _check(gpu, asg, sb, flags=gpu.SCORE_ONLY, kernel="k_asg_lanes")


# ---------------------------------------------------------------------------------------------------------------- directions

@pytest.mark.parametrize("R,mq,nr", [("2", (1, 128), (1, 300)), ("2", (200, 300), (100, 200)), ("4", (129, 256), (50, 300)), ("8", (300, 700), (100, 500))])
def test_directions_against_matrices_and_oracle(gpu, asg, monkeypatch, R, mq, nr):
    monkeypatch.setenv("DPX_R", R)
    sb = _related(zlib.crc32(f"dir{R}{mq}".encode()), 12, mq, nr)
    d = _check(gpu, asg, sb, flags=gpu.KEEP_DIRECTIONS)
    assert d["rows_per_lane"] == int(R) and d["dir_edges"] == "lds"
    with gpu.Batch(ASG, sb.sequences, sb.pairs, *W) as mb, gpu.Batch(ASG, sb.sequences, sb.pairs, *W, flags=gpu.KEEP_DIRECTIONS) as db:
        mb.fill()
        db.fill()
        for x, y in zip(mb.results(), db.results()):
            assert np.array_equal(x, y)
        mb.output_begin(3)
        db.output_begin(3)
        assert db.output_end()[0] == mb.output_end()[0]
    with gpu.Batch(ASG, sb.sequences, sb.pairs, *W, flags=gpu.SCORE_ONLY) as so:
        so.fill()
        assert np.array_equal(so.results()[0], np.array([r["score"] for r in _want(asg, sb, W)]))


def test_directions_with_edge_rows_in_global_memory(gpu, asg):
    """the smallest reference length at which the edge rows (two int32 rows of n + 2 and the staged reference) leave the 64 KiB of LDS"""
    def per_wave(n):
        return 2 * (((n + 2) * 4 + 15) // 16 * 16) + (n + 192 + 15) // 16 * 16
    n = next(x for x in range(7000, 7400) if per_wave(x) > 64 * 1024)
    rng = np.random.default_rng(83)
    ref = (rng.integers(0, 4, n) + 65).astype(np.uint8)
    texts = [(ref.tobytes(), ref[n - 40:].tobytes()), (ref.tobytes(), ref[100:170].tobytes()), (ref[:n - 1].tobytes(), ref[5000:5030].tobytes())]
    below = from_strings(texts[2:])                                      # one column fewer: still in LDS
    with gpu.Batch(ASG, below.sequences, below.pairs, *W, flags=gpu.KEEP_DIRECTIONS) as b:
        assert b.describe()["dir_edges"] == "lds"
    sb = from_strings(texts)
    with gpu.Batch(ASG, sb.sequences, sb.pairs, *W, flags=gpu.KEEP_DIRECTIONS) as b:
        assert b.describe()["dir_edges"] == "global"
    _check(gpu, asg, sb, flags=gpu.KEEP_DIRECTIONS, matrices="all")


# -------------------------------------------------------------------------------------------------------------------- limits

def test_limits(gpu, asg):
    big = from_strings([(b"A" * 1000, b"A" * 1000)])
    w = (40, -1, -3, -1)
    with pytest.raises(gpu.DpxError) as e:
        gpu.Batch(ASG, big.sequences, big.pairs, *w)                          # 40 000 > int16
    assert e.value.status == RANGE
    assert _want(asg, big, w)[0]["score"] == 40000
    _check(gpu, asg, big, w=w, flags=gpu.KEEP_DIRECTIONS, matrices=None)      # ... and correct with directions
    small = from_strings([(b"ACGTACGT", b"CGTA")])
    with pytest.raises(gpu.DpxError) as e:
        gpu.Batch(ASG, small.sequences, small.pairs, *W, flags=gpu.KEEP_DIRECTIONS | gpu.SCORE_ONLY)
    assert e.value.status == INVALID
    with pytest.raises(gpu.DpxError) as e:
        gpu.Batch(ASG, small.sequences, small.pairs, 3, -1, -3, -(1 << 20) - 1)
    assert e.value.status == RANGE
    with pytest.raises(gpu.DpxError) as e:
        gpu.Batch(9, small.sequences, small.pairs, *W)                        # unknown algorithms stay invalid
    assert e.value.status == INVALID
    sb = _related(17, 8, (1, 200), (1, 260))
    _check(gpu, asg, sb, band=7)                                              # a band value is ignored
    _check(gpu, asg, sb, band=0)


# ------------------------------------------------------------------------------------------------------------------ plumbing

def test_packed2_input(gpu, asg):
    sb = _related(41, 20, (1, 300), (1, 300))
    pk, al = gpu.pack2(sb.sequences, sb.pairs)
    _check(gpu, asg, sb, packed2=(pk, al, sb.sequences.size), matrices=None)
    _check(gpu, asg, sb, matrices=None)


def test_one_shot_align_batch(gpu, asg):
    """dpx_align_batch with H, I and D out"""
    sb = _related(42, 4, (1, 120), (1, 150), empties=False)
    lib = gpu.load()
    prm = gpu.capi.Params(ASG, *W, 0)
    n = sb.num_pairs
    sc, er, ec = (np.zeros(n, np.int32) for _ in range(3))
    mats = [[np.zeros((len(sb.qry(p)) + 1, len(sb.ref(p)) + 1), np.int16) for p in range(n)] for _ in range(3)]
    ptrs = [(C.c_void_p * n)(*[m.ctypes.data for m in plane]) for plane in mats]
    seq = np.ascontiguousarray(sb.sequences, dtype=np.uint8)
    prs = np.ascontiguousarray(sb.pairs)
    fn = lib.dpx_align_batch
    saved = fn.argtypes
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t] + [C.c_void_p] * 6
    try:
        rc = fn(C.addressof(prm), seq.ctypes.data, seq.size, prs.ctypes.data, n, sc.ctypes.data, er.ctypes.data, ec.ctypes.data,
                C.addressof(ptrs[0]), C.addressof(ptrs[1]), C.addressof(ptrs[2]))
    finally:
        fn.argtypes = saved
    assert rc == 0
    for p, r in enumerate(_want(asg, sb, W)):
        assert (sc[p], er[p], ec[p]) == (r["score"], *r["end"])
        for k, key in enumerate(("H", "I", "D")):
            assert np.array_equal(mats[k][p].astype(np.int32), r[key]), (p, key)


def test_weight_fuzz_256_symbols(gpu, asg):
    """sign combinations, positive gap weights, mismatch > match; bytes 0..255 including NUL"""
    rng = np.random.default_rng(21)
    combos = [(3, -1, -3, -1), (2, -3, -5, -2), (1, 4, -2, -1), (3, -1, 2, -3), (3, -2, -4, 1), (-1, -2, -3, -1), (5, 0, 0, 0), (2, -1, 0, -1)]
    for w in combos:
        texts = []
        for _ in range(8):
            n, m = int(rng.integers(0, 300)), int(rng.integers(0, 300))
            ref = rng.integers(0, 256, n).astype(np.uint8)
            q = rng.integers(0, 256, m).astype(np.uint8)
            if n and m:
                k = min(n, m) // 2
                q[:k] = ref[n - k:]
                q[0] = 0
                ref[0] = 0
            texts.append((ref.tobytes(), q.tobytes()))
        _check(gpu, asg, from_strings(texts), w=w)


def test_default_rows_explicit_device_and_a_callers_stream(gpu, asg):
    sb = _related(5, 16, (1, 700), (1, 700))
    _check(gpu, asg, sb)
    _check(gpu, asg, sb, device=0, matrices=None, text=False)
    hip = C.CDLL("libamdhip64.so")
    handle = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(handle), 1) == 0 and handle.value   # hipStreamNonBlocking
    want = _want(asg, sb, W)
    with gpu.Batch(ASG, sb.sequences, sb.pairs, *W, device=0) as b:
        b.fill(handle.value)                                                        # no synchronisation between create and this fill
        sc, er, ec = b.results()
        for p, r in enumerate(want):
            assert (sc[p], er[p], ec[p]) == (r["score"], *r["end"]), p
            assert tuple(x.encode("latin-1") for x in b.traceback(p)) == r["lines"], p
    assert hip.hipStreamDestroy(handle) == 0
