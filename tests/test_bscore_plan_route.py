"""What a DPX_LONG_SCORES batch runs (csrc/dpx_plan.cpp), on the CPU through hostcpp/plan_tool: the flag is legal only with exactly one of
DPX_KEEP_BAND_DIRECTIONS (BANW / BAXT) and DPX_KEEP_LOCAL_BAND_DIRECTIONS (BSW / BASW) and then plans that direction batch's geometry
with nothing stored -- kernel=k_bscore_fill / k_lscore_fill, store=0, no traceback=, no matrix=, matrixBytes 0 -- in every mode the
admitted setters bring; every band up to 512 runs the band kernel, covering or not, and 513 is refused; BANW keeps its admission rule;
pairs the int16 DPX_SCORE_ONLY plan refuses with DPX_ERR_RANGE are planned; and the plans without the bit are what they were."""
import subprocess

import pytest

import plan_cases
from bdx_ref import cpl

W = [3, -1, -2, -1]
SCORE_ONLY, DIRS, BAND_DIRS, TWO_PIECE, LOCAL, LOCAL_TWO_PIECE, LONG = 1, 8, 16, 32, 64, 128, 256
INVALID, RANGE, UNSUPPORTED = -1, -4, -8
NO_MODE = (-1, -1, 0)
STORAGE = {"BANW": BAND_DIRS, "BAXT": BAND_DIRS, "BSW": LOCAL, "BASW": LOCAL}
KERNEL = {"BANW": "k_bscore_fill", "BAXT": "k_bscore_fill", "BSW": "k_lscore_fill", "BASW": "k_lscore_fill"}


def case(name, algo, m=300, n=None, pairs=4, flags=None, band=4, env=None, mode=NO_MODE, weights=W):
    c = {"name": name, "algo": algo, "weights": list(weights), "band": band, "flags": STORAGE.get(algo, 0) | LONG if flags is None else flags,
         "env": env or {}, "gen": ["make_batch", pairs, m, n or m, 1]}
    if mode is not None:
        c["mode"] = list(mode)
    return c


@pytest.fixture(scope="module")
def tool():
    return plan_cases.build_tool()


def run(tool, c):
    r = subprocess.run([tool], input=plan_cases.tool_input(c, plan_cases.make_input(c)), capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (c["name"], r.stderr[-2000:])
    return r.stdout.rstrip("\n")


def fields(tool, c):
    line = run(tool, c)
    assert line.startswith("status=0 "), line
    return dict(kv.split("=", 1) for kv in line.split()[1:]), line


def status(tool, c):
    return int(run(tool, c).split()[0].split("=")[1])


def test_statuses_of_the_flag(tool):
    for algo, storage in STORAGE.items():
        assert status(tool, case("alone", algo, flags=LONG)) == INVALID, algo                                # without 0x10 / 0x40
        assert status(tool, case("both", algo, flags=LONG | BAND_DIRS | LOCAL)) == INVALID, algo               # with both
        assert status(tool, case("score_only", algo, flags=LONG | storage | SCORE_ONLY)) == INVALID, algo
        assert status(tool, case("score_only", algo, flags=LONG | SCORE_ONLY)) == INVALID, algo
        assert status(tool, case("with8", algo, flags=LONG | storage | DIRS)) == UNSUPPORTED, algo             # 0x8 on a banded algorithm: its rule wins
        assert status(tool, case("ok", algo)) == 0, algo
    for algo in ("BANW", "BAXT"):
        assert status(tool, case("two", algo, flags=LONG | BAND_DIRS | TWO_PIECE)) == UNSUPPORTED, algo
        assert status(tool, case("wrong", algo, flags=LONG | LOCAL)) == UNSUPPORTED, algo                      # the storage bit of the other family
    assert status(tool, case("two", "BASW", flags=LONG | LOCAL | LOCAL_TWO_PIECE)) == UNSUPPORTED
    for algo in ("BSW", "BASW"):
        assert status(tool, case("wrong", algo, flags=LONG | BAND_DIRS)) == UNSUPPORTED, algo
    for algo in ("LNW", "LSW", "ANW", "ASW", "ASG"):
        for storage in (BAND_DIRS, LOCAL):
            assert status(tool, case("algo", algo, band=0, m=10, flags=LONG | storage)) == UNSUPPORTED, (algo, storage)
        assert status(tool, case("algo", algo, band=0, m=10, flags=LONG)) == INVALID, algo


def test_nothing_moves_without_the_flag(tool):
    for algo, storage in STORAGE.items():  # the storage flags with DPX_SCORE_ONLY keep the planner's answers
        local = storage == LOCAL
        assert status(tool, case("pinned", algo, flags=storage | SCORE_ONLY)) == (INVALID if local else 0), algo  # (0x10 | 0x1 is refused by dpx_batch_create itself)
        got, _ = fields(tool, case("dir", algo, flags=storage))
        assert got["kernel"] == ("k_bdl_fill" if local else "k_bdir_fill") and got["store"] == "1" and got["matrix"] == "banddir4", got


# algorithm x table x z-drop x end bonus; extension mode is BAXT's, so the other three have the two table modes only
ROUTES = [(algo, table, zdrop, bonus) for algo in STORAGE for table in (0, 5) for zdrop in (-1, 100) for bonus in (-1, 5)
          if algo == "BAXT" or (zdrop < 0 and bonus < 0)]


@pytest.mark.parametrize("algo,table,zdrop,bonus", ROUTES)
def test_route_and_describe(tool, algo, table, zdrop, bonus):
    got, line = fields(tool, case("route", algo, band=70, mode=(zdrop, bonus, table)))
    twin, _ = fields(tool, case("twin", algo, band=70, flags=STORAGE[algo], mode=(zdrop, bonus, table)))
    assert (got["algo"], got["kernel_algo"], got["kernel"], got["store"], got["dtype"]) == (algo, algo, KERNEL[algo], "0", "int32"), got
    assert "traceback" not in got and "matrix" not in got, got
    assert (got.get("subst"), got.get("zdrop"), got.get("end_bonus")) == \
        (str(table) if table else None, *((str(zdrop), str(bonus)) if (zdrop >= 0 or bonus >= 0) else (None, None))), got
    # the direction batch's geometry: cells per lane, launch list, waves per workgroup
    for key in ("rows_per_lane", "singles", "couples", "lane_pairs", "waves", "waves_per_workgroup", "seq_input"):
        assert got[key] == twin[key], (key, got, twin)
    assert got["rows_per_lane"] == str(cpl(70))
    info = got["info"].split(",")
    assert info[2] == "0" and int(twin["info"].split(",")[2]) > 0, (got["info"], twin["info"])  # matrixBytes
    tail = line[line.index(" waves_per_workgroup="):line.index(" info=")].split(" ", 2)
    want = ((" zdrop=%d end_bonus=%d" % (zdrop, bonus)) if (zdrop >= 0 or bonus >= 0) else "") + ((" subst=%d" % table) if table else "")
    assert (" " + tail[2] if len(tail) > 2 else "") == want, line


@pytest.mark.parametrize("algo", list(STORAGE))
def test_bands(tool, algo):
    for band, c in [(1, 1), (64, 1), (65, 2), (128, 2), (129, 4), (256, 4), (257, 8), (512, 8)]:
        got, _ = fields(tool, case("cpl", algo, m=600, n=600 + min(band - 1, 41), pairs=3, band=band))
        assert (got["kernel"], got["rows_per_lane"], got["info"].split(",")[2]) == (KERNEL[algo], str(c), "0"), (band, got)
    # a band that covers the matrix runs the band kernel like any other (no unbanded int32 score-only kernel to fall back on) ...
    for m, band in ((20, 20), (20, 21), (20, 512), (100, 512)):
        got, _ = fields(tool, case("cover", algo, m=m, band=band))
        assert (got["kernel"], got["kernel_algo"], got["rows_per_lane"]) == (KERNEL[algo], algo, str(cpl(band))), (m, band, got)
    # ... and 513 is refused, covering or not
    assert status(tool, case("wide", algo, m=20, band=513)) == UNSUPPORTED
    assert status(tool, case("wide", algo, m=600, band=513)) == UNSUPPORTED
    assert status(tool, case("wide", algo, m=600, band=512)) == 0
    # the direction batch's LDS rule: one-wave workgroups first, then refused
    one, _ = fields(tool, case("lds", algo, m=30000, pairs=2, band=64))
    assert one["waves_per_workgroup"] == "1", one
    assert status(tool, case("lds", algo, m=90000, pairs=1, band=64)) == UNSUPPORTED


def test_banw_admission_rule(tool):
    assert status(tool, case("in", "BANW", m=300, n=307, band=8)) == 0        # |m - n| = B - 1
    line = run(tool, case("out", "BANW", m=300, n=308, band=8))                # |m - n| = B
    assert line.startswith("status=%d err=DPX_ALGO_BANW: pair 0" % UNSUPPORTED) and "needs band >= 9" in line, line
    assert status(tool, case("baxt", "BAXT", m=300, n=308, band=8)) == 0      # BAXT has no such rule


def test_pairs_the_int16_score_only_plan_refuses(tool):
    # m + n = 66 000 on BAXT at weights that keep H inside int16: the step key's 65 000 limit
    small = [1, -1, -1, -1]
    assert status(tool, case("keys", "BAXT", m=32000, n=34000, pairs=1, band=64, flags=SCORE_ONLY, weights=small)) == RANGE
    got, _ = fields(tool, case("keys", "BAXT", m=32000, n=34000, pairs=1, band=64, weights=small))
    assert got["kernel"] == "k_bscore_fill" and got["info"].split(",")[2] == "0", got
    # a 700-base pair under table entries 100..127 (the setters check the table's extremes as match / mismatch)
    for algo in STORAGE:
        assert status(tool, case("table", algo, m=700, pairs=1, band=64, flags=SCORE_ONLY, weights=[127, 100, -2, -1])) == RANGE, algo
        assert status(tool, case("table", algo, m=700, pairs=1, band=64, weights=[127, 100, -2, -1])) == 0, algo
    # and the int32 check is still a check: 2^20 * 300 > 2^28
    for algo in STORAGE:
        assert status(tool, case("past", algo, m=300, pairs=1, band=64, weights=[1 << 20, -1, -2, -1])) == RANGE, algo
