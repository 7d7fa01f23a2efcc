"""DPX_KEEP_DIRECTIONS batches (k_linear_dir, k_affine_dir, k_asw_dir, k_asg_dir, k_traceback_dir, k_export_dir) where the layout and the
launch change path: stripe boundaries, partial store groups behind a second stripe, four-wave workgroups (ragged tails, more than 64
KiB of LDS, the fall-back to one wave), edge rows in global memory with several stripes, more than one launch over the reused scratch,
64-cell runs of the walk in every form, and the codes' tie order under every weight set of the matrix fuzz.  tests/dir_check.py compares
every pair bit for bit with the CPU oracles and asserts from dpx_batch_describe the path each case is there for."""
import numpy as np
import pytest

import dir_check as DC
from dpx_gpu_genomics_project_amd.synth import from_strings
from test_gpu_fuzz import WEIGHTS

pytestmark = pytest.mark.gpu

LIN, LOCAL, AFF, GAPPY = (3, -1, -2, -1), (20, -20, -1, -1), (3, -1, -3, -1), (20, -20, -3, -1)
W = {"LNW": LIN, "LSW": LIN, "ANW": AFF, "ASW": AFF, "ASG": AFF}
ROWS = [(algo, r) for algo in DC.ALGOS for r in (2, 4, 8)] + [("LNW", 16)]
KNOBS = ("DPX_R", "DPX_PACKED", "DPX_LANES", "DPX_LANES_PK", "DPX_SPLIT", "DPX_WPB", "DPX_GROUP", "DPX_TB_WALK", "DPX_POOL", "DPX_POOL_GUARD")
SLOTS = 2048  # DPX_DIR_SCRATCH_SLOTS: waves per launch of a batch with global edge rows


@pytest.fixture(scope="module")
def orc(tmp_path_factory):
    return DC.build_oracles(tmp_path_factory.mktemp("dir_edges"))


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _edges(algo):
    return 2 if algo in DC.AFFINE else 1


def _per_wave(algo, n):
    """bytes of one wave's edge rows and staged reference"""
    return _edges(algo) * (((n + 2) * 4 + 15) // 16 * 16) + (n + 192 + 15) // 16 * 16


# ---------------------------------------------------------------------------------------------------------- a. stripe boundaries

@pytest.mark.parametrize("algo,R", ROWS)
def test_stripe_boundaries(gpu, orc, knobs, algo, R):
    """queries of 64R - 1 .. 192R + 1 rows (the last row in lane 63, in lane 0 of the next stripe, one to three stripes) whose paths cross
    the stripe rows: mutated windows with indels against references of 40..100 columns"""
    knobs.setenv("DPX_R", str(R))
    rng = np.random.default_rng(100 + R)
    ms = (64 * R - 1, 64 * R, 64 * R + 1, 128 * R, 128 * R + 1, 192 * R + 1)
    sb = DC.batch_of(rng, [(m, int(rng.integers(40, 101))) for m in ms] + [(m, 40 + (7 * k) % 61) for k, m in enumerate(ms)], indels=4)
    assert sorted(set(DC.stripes(sb, R))) == [1, 2, 3, 4]
    DC.check(gpu, orc, algo, sb, W[algo], R)
    # ... and long references: the path of a query that is a window of its reference crosses every stripe row inside the matrix
    tall = DC.batch_of(rng, [(128 * R + 1, 128 * R + 90), (192 * R + 1, 192 * R + 40)], indels=6)
    DC.check(gpu, orc, algo, tall, W[algo], R)


def _placed_ties():
    core = b"GATTACAGATTACA"
    pad = lambda k: b"T" * k
    return [
        (b"CCCC" + core + b"CCCC", core + core),                 # the same best in two places of the query
        (core + b"GG" + core, core),                             # two columns of one row
        (b"A", b"AA"),                                           # rows 1 and 2: one lane (R = 2)
        (b"AC", b"ACAC"),                                        # rows 2 and 4: two lanes
        (core, pad(130) + core + pad(120) + core),               # two stripes (128 rows per stripe at R = 2)
        (core, pad(1) + core + pad(1) + core),                   # two lanes
        (b"AAAA", b"CCCC"), (b"", b"ACGT"), (b"ACGT", b""), (b"", b""),
        (b"GATTACA", b"GCATGCT"),                                # three cells hold the maximum
    ]


@pytest.mark.parametrize("algo", ["LSW", "ASW"])
def test_start_cell_ties(gpu, orc, knobs, algo):
    """equal maxima in two rows of one lane, two lanes, two stripes and two columns of one row: the first in row-major order is the end"""
    knobs.setenv("DPX_R", "2")
    sb = from_strings(_placed_ties())
    _, want, _ = DC.check(gpu, orc, algo, sb, W[algo], 2)
    for p in (0, 2, 3, 4, 5):  # the maximum is there more than once, in different rows
        H = want[p]["mats"][0]
        rows = np.unique(np.argwhere(H == H.max())[:, 0])
        assert len(rows) >= 2 and want[p]["end"][0] == rows[0], (p, rows)
    H = want[1]["mats"][0]
    assert (H[want[1]["end"][0]] == H.max()).sum() == 2 and want[1]["end"][1] == 14          # two columns of one row
    H = want[4]["mats"][0]
    assert {int(r - 1) // 128 for r in np.unique(np.argwhere(H == H.max())[:, 0])} == {1, 2}  # ... in two stripes


def test_asg_row_m_ties_with_column_0(gpu, orc, knobs):
    """the maximum of row m equals the column-0 border o + m e (row 0 is free: a deletion down any column costs the same): column 0 wins, in
    a lane's first and second register, in the first and in the second stripe"""
    knobs.setenv("DPX_R", "2")
    w = (1, -10, -3, -1)
    sb = from_strings([(b"0000", b"1111"), (b"00000", b"111"), (b"0" * 50, b"1" * 130), (b"0" * 70, b"1" * 257), (b"01" * 20, b"1111")])
    _, want, _ = DC.check(gpu, orc, "ASG", sb, w, 2)
    for p in range(4):
        H = want[p]["mats"][0]
        assert H[-1, 0] == H[-1, 1:].max() == want[p]["score"] and want[p]["end"] == (H.shape[0] - 1, 0), p
    assert want[4]["end"][1] > 0  # (and one pair of the batch ends inside the row)


# ------------------------------------------------------------------------------------------- b. partial store groups, two stripes

@pytest.mark.parametrize("algo,R", ROWS)
def test_partial_groups_behind_a_second_stripe(gpu, orc, knobs, algo, R):
    """m = 64R + 1 and G = 32 / R consecutive reference lengths: every residue of n + 63 modulo the steps of a 16-byte store, with a
    second stripe that starts at chunk Wp / G"""
    knobs.setenv("DPX_R", str(R))
    G = 32 // R
    ns = range(41, 41 + G)
    assert {(n + 63) % G for n in ns} == set(range(G))
    sb = DC.batch_of(np.random.default_rng(200 + R), [(64 * R + 1, n) for n in ns], indels=2)
    assert set(DC.stripes(sb, R)) == {2}
    DC.check(gpu, orc, algo, sb, W[algo], R)


# ------------------------------------------------------------------------------------------------------ c. four-wave workgroups

def _ragged37(rng):
    shapes = [(int(rng.integers(1, 301)), int(rng.integers(1, 201))) for _ in range(37)]
    shapes[0], shapes[5], shapes[36] = (300, 150), (129, 64), (257, 33)
    texts = [DC.window_pair(rng, m, n) for m, n in shapes]
    texts[3] = (b"", texts[3][1])
    texts[17] = (texts[17][0], b"")
    texts[35] = (b"", b"")
    return from_strings(texts)


@pytest.mark.parametrize("algo", DC.ALGOS)
def test_four_waves_ragged_batch(gpu, orc, knobs, algo):
    """37 pairs in 10 workgroups of four waves: waves 1..3 use their own LDS areas, the last workgroup has one wave with a pair"""
    knobs.setenv("DPX_WPB", "4")
    knobs.setenv("DPX_R", "2")
    sb = _ragged37(np.random.default_rng(37))
    assert sb.num_pairs % 4 == 1 and max(DC.stripes(sb, 2)) == 3 and min(DC.stripes(sb, 2)) == 0
    DC.check(gpu, orc, algo, sb, W[algo], 2, wpb=4)


@pytest.mark.parametrize("algo", DC.ALGOS)
def test_four_waves_above_64_kib_of_lds(gpu, orc, knobs, algo):
    """references of about 4000 (linear) / 2000 (affine) columns: four waves need more than the 64 KiB a kernel gets by default"""
    knobs.setenv("DPX_WPB", "4")
    knobs.setenv("DPX_R", "2")
    n = 2000 if algo in DC.AFFINE else 4000
    assert 64 * 1024 < 4 * _per_wave(algo, n) <= 160 * 1024
    rng = np.random.default_rng(64)
    sb = DC.batch_of(rng, [(150, n), (40, n - 1), (129, n - 17), (7, 300), (128, n - 2), (90, n // 2)])
    assert sb.num_pairs % 4 == 2 and max(DC.stripes(sb, 2)) == 2
    DC.check(gpu, orc, algo, sb, W[algo], 2, wpb=4)


@pytest.mark.parametrize("algo", DC.ALGOS)
def test_four_waves_fall_back_to_one(gpu, orc, knobs, algo):
    """references of about 9000 (linear) / 4700 (affine) columns: four waves would pass 160 KiB, one wave's edge rows still fit LDS"""
    knobs.setenv("DPX_WPB", "4")
    knobs.setenv("DPX_R", "2")
    n = 4700 if algo in DC.AFFINE else 9000
    assert 4 * _per_wave(algo, n) > 160 * 1024 and _per_wave(algo, n) <= 64 * 1024
    sb = DC.batch_of(np.random.default_rng(160), [(140, n), (33, n - 5), (129, 77)])
    DC.check(gpu, orc, algo, sb, W[algo], 2, wpb=1, edges="lds", matrix="auto")


# ------------------------------------------------------------------------------------- d. global edge rows with several stripes

@pytest.mark.parametrize("algo", DC.ALGOS)
def test_global_edge_rows_three_stripes(gpu, orc, knobs, algo):
    """the smallest reference length whose edge rows leave LDS, under queries of three stripes at 2 rows per lane: lane 63 writes the
    stripe's bottom row to memory and the next stripe's lane 0 reads it back"""
    knobs.setenv("DPX_R", "2")
    n = DC.global_threshold(_edges(algo))
    assert 13000 < n < 13100 if _edges(algo) == 1 else 7200 < n < 7300
    assert _per_wave(algo, n) > 64 * 1024 >= _per_wave(algo, n - 1)
    rng = np.random.default_rng(n)
    sb = DC.batch_of(rng, [(300, n), (257, n - 5), (256, n - 16)], indels=6)
    assert DC.stripes(sb, 2) == [3, 3, 2]
    DC.check(gpu, orc, algo, sb, W[algo], 2, edges="global", matrix="auto")
    below = DC.batch_of(rng, [(300, n - 1)], indels=6)               # one column fewer: the same three stripes with the rows in LDS
    DC.check(gpu, orc, algo, below, W[algo], 2, edges="lds", matrix="auto")


def test_global_edge_rows_lnw_two_stripes_of_16_rows(gpu, orc):
    """LNW at its default 16 rows per lane (two registers of codes per step)"""
    n = DC.global_threshold(1)
    rng = np.random.default_rng(16)
    sb = DC.batch_of(rng, [(1100, n), (1025, n - 3)], indels=6)
    assert DC.stripes(sb, 16) == [2, 2]
    DC.check(gpu, orc, "LNW", sb, LIN, 16, edges="global", matrix="auto")
    below = DC.batch_of(rng, [(1100, n - 1)], indels=6)
    DC.check(gpu, orc, "LNW", below, LIN, 16, edges="lds", matrix="auto")


# ----------------------------------------------------------------------------------------------------- e. more than one launch

@pytest.mark.parametrize("algo", ["LSW", "ANW", "ASG"])
def test_more_than_one_launch(gpu, orc, knobs, algo):
    """2100 pairs of two stripes each, one of them with its reference at the global threshold: the whole batch runs with global edge rows,
    2048 waves in the first launch and 52 in the second, which takes the scratch areas the first one used"""
    knobs.setenv("DPX_R", "2")
    count = 2100
    n_long = DC.global_threshold(_edges(algo))
    rng = np.random.default_rng(2100)
    shapes = [(int(rng.integers(129, 201)), int(rng.integers(10, 41))) for _ in range(count)]
    shapes[777] = (shapes[777][0], n_long)
    sb = DC.batch_of(rng, shapes, indels=2)
    assert sb.num_pairs > SLOTS and set(DC.stripes(sb, 2)) == {2}
    assert sum(_per_wave(algo, n) > 64 * 1024 for _, n in shapes) == 1
    cells = np.array([m * n for m, n in shapes])
    smallest = np.argsort(cells, kind="stable")[:64]                  # (whatever the launch order, the second launch holds the smallest pairs)
    picks = sorted(set(range(0, count, 16)) | set(smallest.tolist()) | {777})
    DC.check(gpu, orc, algo, sb, W[algo], 2, edges="global", planes=picks, matrix="auto")


# -------------------------------------------------------------------------------------------------------- f. runs in the walk

GAP_W = {"LNW": LIN, "LSW": LOCAL, "ANW": AFF, "ASW": GAPPY, "ASG": GAPPY}
GAP_RUNS = (63, 64, 65, 127, 128, 129, 200)


# gapOpen = 0: the open term is never below the extend term, so every step of a gap opens anew (the affine walker leaves its gap state after
# every step); ANW's set is LNW's 3/-1/-2, the other one LSW's 20/-20/-1
GAP_W_OPENING = {"ANW": (3, -1, 0, -2), "ASW": (20, -20, 0, -1), "ASG": (20, -20, 0, -1)}
GAP_CASES = [(algo, "extending") for algo in DC.ALGOS] + [(algo, "opening") for algo in GAP_W_OPENING]


@pytest.mark.parametrize("algo,form", GAP_CASES)
def test_gap_runs(gpu, orc, knobs, algo, form):
    """one gap of exactly L around 64 and 128 steps, horizontal and vertical: the walk takes it in trips of 64 lanes (the affine walker stays
    in its gap state from one trip to the next while the cells extend, and takes one step per trip where every cell opens), a vertical
    one crosses the stripe row"""
    knobs.setenv("DPX_R", "2")
    w = GAP_W[algo] if form == "extending" else GAP_W_OPENING[algo]
    rng = np.random.default_rng(6)
    acg = np.frombuffer(b"ACG", np.uint8)
    texts = []
    for L in GAP_RUNS:
        x, z = rng.choice(acg, 40).tobytes(), rng.choice(acg, 40).tobytes()
        texts += [(x + b"T" * L + z, x + z), (x + z, x + b"T" * L + z)]
    sb = from_strings(texts)
    want = DC.want_of(orc, algo, sb, w)
    for p, r in enumerate(want):                                       # the oracle's own lines hold the run
        L = GAP_RUNS[p // 2]
        gapped = r["lines"][2] if p % 2 == 0 else r["lines"][0]
        assert b"_" * L in gapped and b"_" * (L + 1) not in gapped and len(r["lines"][0]) == 80 + L, (algo, p, L, r["lines"])
        if algo in DC.AFFINE:                                          # ... and its gap plane the run of GAP_EXTEND (2) the walker follows, or none
            plane = r["dirs"][1] if p % 2 == 0 else r["dirs"][2]
            line = plane[40] if p % 2 == 0 else plane[:, 40]          # the gap runs along row / column 40, behind X
            run = line[41:41 + L]
            assert np.all(run[1:] == 2) if form == "extending" else not (r["dirs"][1] == 2).any() and not (r["dirs"][2] == 2).any(), (algo, p, L, run.tolist())
    DC.check(gpu, orc, algo, sb, w, 2, want=want)


DECOY_W = {"ANW": (3, -1, -5, -1), "ASW": (20, -20, -50, -1), "ASG": (20, -20, -50, -1)}


@pytest.mark.parametrize("algo", DC.AFFINE)
def test_gap_state_is_kept_where_h_points_elsewhere(gpu, orc, knobs, algo):
    """a gap of 129 / 200 steps whose cell 64 (and 128) steps in -- where a trip of the walk ends -- has an H that comes from the diagonal:
    the short side's base before the gap mismatches on the path and matches a base planted inside the long side's run.  The path stays in
    the gap (opening twice costs more than the mismatch), so the walker must go on in its gap state and not read H's move there"""
    knobs.setenv("DPX_R", "2")
    w = DECOY_W[algo]
    rng = np.random.default_rng(64)
    acg = np.frombuffer(b"ACG", np.uint8)
    texts, decoys = [], []
    for L in (129, 200):
        x, z = rng.choice(acg, 40).tobytes(), rng.choice(acg, 40).tobytes()
        other = bytes([next(c for c in b"ACG" if c != x[-1])])
        run = bytearray(b"T" * L)
        at = [40 + L - 64 * k for k in range(1, 4) if 40 + L - 64 * k > 40]   # 1-based positions in the long side where a trip ends
        for pos in at:
            run[pos - 41] = x[-1]
        long, short = x[:-1] + other + bytes(run) + z, x + z
        texts += [(long, short), (short, long)]
        decoys += [at, at]
    sb = from_strings(texts)
    want = DC.want_of(orc, algo, sb, w)
    for p, r in enumerate(want):
        L = (129, 200)[p // 2]
        gapped = r["lines"][2] if p % 2 == 0 else r["lines"][0]
        assert b"_" * L in gapped and b"_" * (L + 1) not in gapped and len(r["lines"][0]) == 80 + L, (algo, p, r["lines"])
        for pos in decoys[p]:   # H of the trip's last cell is a MATCH, its gap cell extends: the planes disagree about the way on
            cell = (40, pos) if p % 2 == 0 else (pos, 40)
            assert r["dirs"][0][cell] == 1 and r["dirs"][1 if p % 2 == 0 else 2][cell] == (2 if pos > 41 else 1), (algo, p, pos)   # (41: the gap's first cell opens)
    DC.check(gpu, orc, algo, sb, w, 2, want=want)


@pytest.mark.parametrize("algo", DC.ALGOS)
def test_diagonal_runs_and_runs_cut_by_a_border(gpu, orc, knobs, algo):
    """identical strings of 63 .. 300 bases (diagonal runs of whole trips, across the stripe rows 128 and 256); runs that end on row or column
    0 inside a trip: identical 10-mers, one row against 200 columns and 200 rows against one column (LNW's and ANW's border tails)"""
    knobs.setenv("DPX_R", "2")
    rng = np.random.default_rng(9)
    texts = []
    for L in (63, 64, 65, 128, 129, 300):
        s = DC.ACGT[rng.integers(0, 4, L)].tobytes()
        texts.append((s, s))
    ten = DC.ACGT[rng.integers(0, 4, 10)].tobytes()
    long = DC.ACGT[rng.integers(0, 4, 200)].tobytes()
    texts += [(ten, ten), (long, long[120:121]), (long[77:78], long), (long, b"T" if long[0:1] != b"T" else b"A"), (b"A" * 200, b"C"), (b"C", b"A" * 200)]
    sb = from_strings(texts)
    w = W[algo]
    want = DC.want_of(orc, algo, sb, w)
    for p, L in enumerate((63, 64, 65, 128, 129, 300, 10)):
        assert want[p]["lines"][1] == b"*" * L and want[p]["score"] == w[0] * L, (algo, p)
    if algo in ("LNW", "ANW"):  # global: the rest of the long side is a border tail of 199 gaps
        for p in (7, 8, 9, 10, 11):
            assert len(want[p]["lines"][0]) in (200, 201) and want[p]["lines"][1].count(b" ") >= 199, (algo, p, want[p]["lines"])
    DC.check(gpu, orc, algo, sb, w, 2, want=want)


# ------------------------------------------------------------------------------------------------------- g. weights and ties

ASW_COMBOS = [(3, -1, -3, -1), (2, -3, -5, -2), (1, 4, -2, -1), (3, -1, 2, -3), (3, -2, -4, 1), (-1, -2, -3, -1), (5, 0, 0, 0), (2, -1, 0, -1)]  # test_weight_fuzz_256_symbols
TIE_WEIGHTS = {"LNW": WEIGHTS, "LSW": WEIGHTS, "ANW": WEIGHTS, "ASW": ASW_COMBOS, "ASG": ASW_COMBOS}
TIE_CASES = [pytest.param(algo, w, id=f"{algo}-{'_'.join(map(str, w))}") for algo in DC.ALGOS for w in TIE_WEIGHTS[algo]]
# weight sets under which a tie class cannot occur, by (algorithm, weights): class index (from 0) -> why.  The test asserts that the oracle
# finds none there, so an entry that stops being true fails too.
_OPEN_ABOVE_0 = "H >= I and H >= D in every cell, so with gapOpen > 0 the open term H + o + e is above the extend term"
NO_SUCH_TIE = {
    ("LNW", (1, -2, 1, -3)): {0: "a gap step pays +1 and a diagonal step at most +1 for two: H[i][j] = i + j, up = i + j, the diagonal term <= i + j - 1"},
    ("ANW", (1, -2, 1, -3)): {2: _OPEN_ABOVE_0},
    ("ASW", (3, -1, 2, -3)): {2: _OPEN_ABOVE_0},
    ("ASG", (3, -1, 2, -3)): {2: _OPEN_ABOVE_0},
    # no positive weight under the zero floor: H = 0, I = D = o + e = -4 in every cell, the diagonal term is -1 or -2, the extend term -5
    ("ASW", (-1, -2, -3, -1)): {0: "H = 0 everywhere", 1: "H = 0 everywhere", 2: "H = 0 everywhere"},
    # row 0 is free, so D[i][j] >= o + i e = -3 - i in every column, while a horizontal gap of k starts from H[i][j-k] <= -i and costs
    # 3 + k more: I <= -i - 4 < D
    ("ASG", (-1, -2, -3, -1)): {1: "I < D in every cell"},
}


def _tie_texts():
    rng = np.random.default_rng(77)
    texts = []
    for alphabet in (DC.ACGT, np.arange(256, dtype=np.uint8), np.array([0, 255], np.uint8)):
        for k in range(6):
            m, n = int(rng.integers(0, 301)), int(rng.integers(0, 301))
            if k < 4:   # related, with indels
                texts.append(DC.window_pair(rng, m, n, alphabet))
            else:
                texts.append((rng.choice(alphabet, n).astype(np.uint8).tobytes(), rng.choice(alphabet, m).astype(np.uint8).tobytes()))
    texts.append(DC.window_pair(rng, 300, 280))                        # (pins the rows per lane: 8)
    texts += [(b"A" * 40, b"A" * 40), (b"A" * 37, b"A" * 40), (b"A" * 70, b"A" * 130), (b"A" * 30, b"C" * 30), (b"C" * 33, b"A" * 30), (b"AC" * 20, b"CA" * 20)]
    two = lambda: rng.integers(65, 67, int(rng.integers(20, 90))).astype(np.uint8).tobytes()
    texts += [(two(), two()) for _ in range(6)]
    texts += [(b"", b"ACGT"), (b"ACGT", b""), (b"", b"")]
    return from_strings(texts)


_TIE_SB = []


@pytest.mark.parametrize("algo,w", TIE_CASES)
def test_weights_and_ties(gpu, orc, algo, w):
    """zero weights, positive gaps, mismatch above match, over ACGT, all 256 bytes and {0, 255}, homopolymers and two-letter strings: every
    cell where two candidates tie takes the move the reference's order gives -- and the ties are there (counted from the oracle's matrices)"""
    if not _TIE_SB:
        _TIE_SB.append(_tie_texts())
    sb = _TIE_SB[0]
    want = DC.want_of(orc, algo, sb, w)
    total = np.zeros(2 if algo in ("LNW", "LSW") else 3, np.int64)
    for p, r in enumerate(want):
        total += DC.tie_counts(algo, r, w, sb.ref(p), sb.qry(p))
    exempt = NO_SUCH_TIE.get((algo, tuple(w)), {})
    for k, cnt in enumerate(total):
        assert (cnt == 0) if k in exempt else (cnt >= 1), (algo, w, "tie class", k + 1, total.tolist())
    DC.check(gpu, orc, algo, sb, w, 8, want=want)
