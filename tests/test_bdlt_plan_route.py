"""What a DPX_KEEP_LOCAL_BAND_DIRECTIONS batch of BSW / BASW runs under a substitution table (dpx_batch_set_local_direction_table;
csrc/dpx_plan.cpp), on the CPU through hostcpp/plan_tool's `mode` line: k_bdlt_fill / k_bdl_traceback / bdl:0 / banddir4 with subst=
between them, the pool unchanged, a covering band still a dir4 batch, no mode what tests/test_bdl_plan_route.py sees, one-wave workgroups
where four waves' strings and table images do not fit LDS, and 0 waves (the setter's refusal) where one wave's do not."""
import pytest

import plan_cases
from test_bdl_plan_route import NO_MODE, case, fields

TABLE = (-1, -1, 24)
LDS, IMAGE = 160 * 1024, 1280


@pytest.fixture(scope="module")
def tool():
    return plan_cases.build_tool()


def staged(m, n):
    """one wave's staged strings of a band-direction batch (csrc/dpx_plan.cpp, main_lds: the query with 64 + 32 bytes of slack, the
    reference with 128 + 16, each rounded up to 16)"""
    up = lambda v: -(-v // 16) * 16
    return up(m + 96) + up(n + 144)


@pytest.mark.parametrize("algo", ["BSW", "BASW"])
def test_a_table_runs_the_table_fill_and_nothing_else_changes(tool, algo):
    plain, _ = fields(tool, case("bdlt", algo, m=600, n=641, band=128))
    got, line = fields(tool, case("bdlt", algo, m=600, n=641, band=128, mode=TABLE))
    assert (got["algo"], got["kernel_algo"], got["kernel"], got["traceback"], got["walk"], got["matrix"], got["subst"]) == \
        (algo, algo, "k_bdlt_fill", "k_bdl_traceback", "bdl:0", "banddir4", "24"), got
    assert line[line.index(" traceback="):line.index(" info=")] == " traceback=k_bdl_traceback subst=24 matrix=banddir4", line  # k_bdx_fill's field order
    assert plain["kernel"] == "k_bdl_fill" and "subst" not in plain
    for key in got:  # the pool (info), the plan (state) and every other field
        if key not in ("kernel", "subst"):
            assert got[key] == plain[key], key
    for walk in (0, 1, 2):
        assert fields(tool, case("bdlt", algo, mode=TABLE, env={"DPX_TB_WALK": walk}))[0]["walk"] == "bdl:0"


@pytest.mark.parametrize("algo,kalgo", [("BSW", "LSW"), ("BASW", "ASW")])
def test_a_covering_band_stays_a_direction_batch(tool, algo, kalgo):
    got, _ = fields(tool, case("cover", algo, m=20, band=20, mode=NO_MODE))
    assert got["kernel_algo"] == kalgo and got["matrix"] == "dir4" and got["kernel"] in ("k_linear_dir", "k_asw_dir") and got["walk"] == "dir:0", got
    tabled, _ = fields(tool, case("cover", algo, m=20, band=20, mode=TABLE))  # (the setter refuses it; the planner never names the table fill)
    assert tabled["kernel"] == got["kernel"] and tabled["matrix"] == "dir4" and tabled["walk"] == "dir:0", tabled


@pytest.mark.parametrize("algo", ["BSW", "BASW"])
def test_no_mode_is_the_plain_local_batch(tool, algo):
    got, line = fields(tool, case("bdl", algo, mode=NO_MODE))
    assert (got["kernel"], got["traceback"], got["walk"], got["matrix"]) == ("k_bdl_fill", "k_bdl_traceback", "bdl:0", "banddir4"), got
    assert line[line.index(" traceback="):line.index(" info=")] == " traceback=k_bdl_traceback matrix=banddir4", line
    bare, bare_line = fields(tool, case("bdl", algo, mode=None))
    assert "walk" not in bare and line.startswith(bare_line)


def test_four_waves_become_one_where_the_images_no_longer_fit(tool):
    """four waves x (staged strings + 1280 B) against 160 KiB: 20 000 x 20 000 keeps four waves plain and drops to one under the table
    (DPX_WPB=4: a batch of few pairs runs one-wave workgroups of its own accord)"""
    wpb = {"DPX_WPB": 4}
    L = 20000
    assert 4 * staged(L, L) <= LDS < 4 * (staged(L, L) + IMAGE)
    for algo in ("BSW", "BASW"):
        plain, _ = fields(tool, case("edge", algo, m=L, pairs=4, band=64, mode=NO_MODE, env=wpb))
        got, _ = fields(tool, case("edge", algo, m=L, pairs=4, band=64, mode=TABLE, env=wpb))
        assert (plain["waves_per_workgroup"], got["waves_per_workgroup"]) == ("4", "1"), (plain, got)
        assert got["kernel"] == "k_bdlt_fill" and got["info"] == plain["info"] and got["state"] == plain["state"]
    # the last length whose four slices fit with the image keeps four waves
    fit = max(x for x in range(19000, 20000) if 4 * (staged(x, x) + IMAGE) <= LDS)
    assert 4 * (staged(fit + 16, fit + 16) + IMAGE) > LDS
    assert fields(tool, case("edge", "BASW", m=fit, pairs=4, band=64, mode=TABLE, env=wpb))[0]["waves_per_workgroup"] == "4"
    assert fields(tool, case("edge", "BASW", m=fit + 16, pairs=4, band=64, mode=TABLE, env=wpb))[0]["waves_per_workgroup"] == "1"
    # strings that already run one-wave workgroups stay there
    assert fields(tool, case("edge", "BASW", m=30000, pairs=2, band=64, mode=TABLE, env=wpb))[0]["waves_per_workgroup"] == "1"


def test_no_room_for_the_image_is_zero_waves(tool):
    """strings that fit one wave alone but not with the image: the planner answers 0 waves, which is the setter's DPX_ERR_UNSUPPORTED"""
    L = 81500
    assert staged(L, L) <= LDS < staged(L, L) + IMAGE
    plain, _ = fields(tool, case("full", "BASW", m=L, pairs=1, band=64, mode=NO_MODE))
    got, _ = fields(tool, case("full", "BASW", m=L, pairs=1, band=64, mode=TABLE))
    assert (plain["waves_per_workgroup"], got["waves_per_workgroup"]) == ("1", "0"), (plain, got)
    room = max(x for x in range(80000, L) if staged(x, x) + IMAGE <= LDS)
    assert fields(tool, case("full", "BSW", m=room, pairs=1, band=64, mode=TABLE))[0]["waves_per_workgroup"] == "1"
