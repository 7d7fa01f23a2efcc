"""What a DPX_KEEP_LOCAL_BAND_DIRECTIONS | DPX_LOCAL_TWO_PIECE_GAPS batch of BASW runs (csrc/dpx_plan.cpp), on the CPU through
hostcpp/plan_tool: k_lb2_fill / k_lb2_traceback / lb2:0 / banddir8 with ` gap2=` behind the layout and ` subst=` in front of it under a
table, the pool sized by the byte layout, band 256 admitted and 257 unsupported, a covering band still on the band kernel, every flag
combination of the definition, and the routes of the batches that existed before printing exactly what they printed."""
import pytest

import plan_cases
from test_bd2_plan_route import fields, run
from test_bdl_plan_route import BAND_DIRS, DIRS, LOCAL, NO_MODE, SCORE_ONLY, TWO_PIECE, W

LOCAL2 = 0x80
INVALID, UNSUPPORTED = -1, -8
TABLE = (-1, -1, 24)


def case(name, algo="BASW", m=300, n=None, pairs=4, flags=LOCAL | LOCAL2, band=4, env=None, mode=NO_MODE):
    c = {"name": name, "algo": algo, "weights": W, "band": band, "flags": flags, "env": env or {}, "gen": ["make_batch", pairs, m, n or m, 1]}
    if mode is not None:
        c["mode"] = list(mode)
    return c


def status(tool, c):
    return int(run(tool, c).split()[0].split("=")[1])


@pytest.fixture(scope="module")
def tool():
    return plan_cases.build_tool()


def test_the_flag_runs_the_two_piece_local_kernels(tool):
    got, line = fields(tool, case("lb2"), gap2=(-24, -1))
    assert (got["algo"], got["kernel_algo"], got["kernel"], got["traceback"], got["walk"], got["matrix"], got["gap2"]) == \
        ("BASW", "BASW", "k_lb2_fill", "k_lb2_traceback", "lb2:0", "banddir8", "-24,-1"), got
    assert (got["dtype"], got["rows_per_lane"], got["store"], got["couples"], got["lane_pairs"]) == ("int32", "1", "1", "0", "0"), got
    assert line[line.index(" traceback="):line.index(" info=")] == " traceback=k_lb2_traceback matrix=banddir8 gap2=-24,-1", line
    assert fields(tool, case("lb2"))[0]["gap2"] == "-2,-1"  # until the setter is called: piece 1
    for walk in (0, 1, 2):  # one walk: DPX_TB_WALK has no effect
        assert fields(tool, case("lb2", env={"DPX_TB_WALK": walk}))[0]["walk"] == "lb2:0"
    # under a table: the same kernel, ` subst=` in k_bdx_fill's field order, the pool and the plan unchanged
    tabled, tline = fields(tool, case("lb2", mode=TABLE), gap2=(-24, -1))
    assert tline[tline.index(" traceback="):tline.index(" info=")] == " traceback=k_lb2_traceback subst=24 matrix=banddir8 gap2=-24,-1", tline
    for key in tabled:
        if key != "subst":
            assert tabled[key] == got[key], key


@pytest.mark.parametrize("band,cpl", [(1, 1), (64, 1), (65, 2), (128, 2), (129, 4), (256, 4)])
def test_the_pool_is_sized_by_the_byte_layout(tool, band, cpl):
    m, n = 600, 641
    got, _ = fields(tool, case("chunks", m=m, n=n, pairs=3, band=band))
    gd = 16 // cpl
    assert got["rows_per_lane"] == str(cpl)
    assert int(got["info"].split(",")[2]) == 3 * -(-(m + n - 1) // gd) * 1024, got["info"]
    plain, _ = fields(tool, case("chunks", m=m, n=n, pairs=3, band=band, flags=LOCAL))
    assert int(plain["info"].split(",")[2]) == 3 * -(-(m + n - 1) // (2 * gd)) * 1024  # twice k_bdl_fill's bytes


def test_band_limit_and_covering_bands(tool):
    assert status(tool, case("wide", m=600, band=256)) == 0
    assert status(tool, case("wide", m=600, band=257)) == UNSUPPORTED
    assert status(tool, case("wide", m=20, band=257)) == UNSUPPORTED  # covering or not
    assert status(tool, case("wide", m=600, band=512, flags=LOCAL)) == 0  # (the one-piece batch goes to 512)
    # a covering band stays on the band kernel: ASW has no second piece
    for band in (20, 21, 256):
        got, _ = fields(tool, case("cover", m=20, band=band))
        assert (got["kernel_algo"], got["kernel"], got["traceback"], got["matrix"], got["walk"]) == ("BASW", "k_lb2_fill", "k_lb2_traceback", "banddir8", "lb2:0"), got
    plain, _ = fields(tool, case("cover", m=20, band=20, flags=LOCAL))
    assert (plain["kernel_algo"], plain["kernel"], plain["matrix"]) == ("ASW", "k_asw_dir", "dir4"), plain


def test_flag_combinations(tool):
    for algo in ("BASW", "BSW", "ASW", "BANW", "LSW"):
        assert status(tool, case("alone", algo, flags=LOCAL2)) == INVALID, algo  # 0x80 without 0x40
    for extra in (SCORE_ONLY, BAND_DIRS, TWO_PIECE, BAND_DIRS | TWO_PIECE):
        assert status(tool, case("with", flags=LOCAL | LOCAL2 | extra)) == INVALID, extra
        assert status(tool, case("with", flags=LOCAL2 | extra)) == INVALID, extra
    assert status(tool, case("with8", flags=LOCAL | LOCAL2 | DIRS)) == UNSUPPORTED
    for algo in ("BSW", "BANW", "ASW", "LNW", "LSW", "ANW", "ASG", "BAXT"):  # BASW's alone, BSW included
        assert status(tool, case("algo", algo, band=8, m=10)) == UNSUPPORTED, algo
    # the pins of the flags that existed stay
    assert status(tool, case("pin", flags=LOCAL | TWO_PIECE)) == INVALID
    assert status(tool, case("pin", "BSW", flags=LOCAL | TWO_PIECE)) == INVALID


# hostcpp/plan_tool's lines for four batches that existed before the flag, recorded from the commit that introduced it (m = 600, n = 641,
# four pairs, band 128, weights 3 / -1 / -2 / -1)
BEFORE = {
    "local": "status=0 algo=BASW kernel_algo=BASW kernel=k_bdl_fill dtype=int32 rows_per_lane=2 store=1 couples=0 lane_pairs=0 waves=0 singles=4 row_tags=0 seq_input=bytes waves_per_workgroup=1 traceback=k_bdl_traceback matrix=banddir4 info=4,1538400,319488,287340 state=a94d419b00670e58 walk=bdl:0",
    "local_table": "status=0 algo=BASW kernel_algo=BASW kernel=k_bdlt_fill dtype=int32 rows_per_lane=2 store=1 couples=0 lane_pairs=0 waves=0 singles=4 row_tags=0 seq_input=bytes waves_per_workgroup=1 traceback=k_bdl_traceback subst=24 matrix=banddir4 info=4,1538400,319488,287340 state=a94d419b00670e58 walk=bdl:0",
    "two_piece": "status=0 algo=BAXT kernel_algo=BAXT kernel=k_bd2_fill dtype=int32 rows_per_lane=2 store=1 couples=0 lane_pairs=0 waves=0 singles=4 row_tags=0 seq_input=bytes waves_per_workgroup=1 traceback=k_bd2_traceback matrix=banddir8 gap2=-2,-1 info=4,1538400,634880,569600 state=b4865cde0682d257 walk=bd2:0",
    "plain": "status=0 algo=BASW kernel_algo=BASW kernel=k_basw_fill dtype=int32 rows_per_lane=2 store=1 couples=0 lane_pairs=0 waves=0 singles=4 row_tags=0 seq_input=bytes waves_per_workgroup=1 traceback=k_basw_traceback_wave info=4,1538400,3809280,3392220 state=a3b52c3ff85eb9dd walk=basw:2",
}


def test_the_batches_that_existed_print_what_they_printed(tool):
    shape = dict(m=600, n=641, band=128)
    assert run(tool, case("before", flags=LOCAL, **shape)) == BEFORE["local"]
    assert run(tool, case("before", flags=LOCAL, mode=TABLE, **shape)) == BEFORE["local_table"]
    assert run(tool, case("before", "BAXT", flags=BAND_DIRS | TWO_PIECE, **shape)) == BEFORE["two_piece"]
    assert run(tool, case("before", flags=0, **shape)) == BEFORE["plain"]
    # and the new batch of the same pairs: the two-piece BAXT batch's pool, the one-piece local batch's strings
    got, _ = fields(tool, case("before", **shape))
    assert got["info"].split(",")[2] == "634880" and got["kernel"] == "k_lb2_fill"
