"""What a band-direction batch runs under dpx_batch_set_direction_scoring (csrc/dpx_plan.cpp: dpx_plan_route, dpx_plan_bdx_waves), on the
CPU through hostcpp/plan_tool with a `mode` line: any mode gives k_bdx_fill with the one walk of band-direction batches, no mode gives
k_bdir_fill as before, the mode fields are printed as a matrix batch prints them, and a table shrinks the workgroup to one wave exactly
when four waves' strings fit one workgroup's LDS without the table image and not with it."""
import pytest

import plan_cases

W = [3, -1, -2, -1]
BAND_DIRS = 16
LDS_MAX, IMAGE = 160 * 1024, 1280  # one workgroup's LDS; DPX_SUBST_IMAGE_BYTES per wave


def case(name, algo, mode, env=None, m=8, pairs=4, flags=BAND_DIRS, band=4):
    return {"name": name, "algo": algo, "weights": W, "band": band, "flags": flags, "env": env or {}, "gen": ["make_batch", pairs, m, m, 1],
            "mode": list(mode)}


BAXT_MODES = [(-1, -1, 5), (-1, 3, 0), (2, 3, 0), (-1, 3, 5), (2, 3, 5)]  # table; bonus; drop; table + bonus; table + drop


@pytest.fixture(scope="module")
def tool():
    return plan_cases.build_tool()


def fields(tool, c):
    line = plan_cases.run_tool(tool, c)
    assert line.startswith("status=0 "), line
    return dict(kv.split("=", 1) for kv in line.split()[1:]), line


@pytest.mark.parametrize("knob", [None, 0, 2])
@pytest.mark.parametrize("algo,mode", [("BANW", (-1, -1, 5))] + [("BAXT", m) for m in BAXT_MODES])
def test_any_mode_runs_k_bdx_fill(tool, algo, mode, knob):
    got, line = fields(tool, case("bdx", algo, mode, env={} if knob is None else {"DPX_TB_WALK": knob}))
    assert (got["kernel"], got["traceback"], got["walk"], got["matrix"]) == ("k_bdx_fill", "k_bdir_traceback", "bdir:0", "banddir4"), got
    z, e, alphabet = mode
    assert (got.get("zdrop"), got.get("end_bonus")) == ((str(z), str(e)) if (z >= 0 or e >= 0) else (None, None)), got
    assert got.get("subst") == (str(alphabet) if alphabet else None), got
    # ... in a matrix batch's order: ` zdrop= end_bonus=`, then ` subst=`, then the batch's own ` matrix=`
    tail = line[line.index(" traceback="):line.index(" info=")]
    want = " traceback=k_bdir_traceback" + (f" zdrop={z} end_bonus={e}" if (z >= 0 or e >= 0) else "") + (f" subst={alphabet}" if alphabet else "")
    assert tail == want + " matrix=banddir4", tail
    matrix, mline = fields(tool, case("matrix", algo, mode, flags=0))
    assert mline[mline.index(" traceback="):mline.index(" info=")].split()[1:] == want.split()[1:]


@pytest.mark.parametrize("algo", ["BANW", "BAXT"])
def test_no_mode_is_k_bdir_fill(tool, algo):
    got, _ = fields(tool, case("plain", algo, (-1, -1, 0)))
    assert (got["kernel"], got["traceback"], got["walk"]) == ("k_bdir_fill", "k_bdir_traceback", "bdir:0"), got
    assert "zdrop" not in got and "subst" not in got


def test_a_table_shrinks_the_workgroup_only_when_four_images_do_not_fit(tool):
    """main_lds (dpx_plan.cpp): a band kernel's wave stages its query in align16(m + 64 + 32) bytes and its reference in
    align16(n + 128 + 16).  At m = n = 20 200 that is 20 304 + 20 352 = 40 656 bytes: four waves take 162 624 of the 163 840 bytes, four
    waves with their 1280-byte table images 167 744."""
    m = 20200
    per_wave = -(-(m + 96) // 16) * 16 + -(-(m + 144) // 16) * 16
    assert 4 * per_wave <= LDS_MAX < 4 * (per_wave + IMAGE) and per_wave + IMAGE <= LDS_MAX
    kw = dict(env={"DPX_WPB": 4}, m=m, pairs=1, band=16)
    for mode, waves in (((-1, -1, 0), "4"), ((2, 3, 0), "4"), ((-1, -1, 5), "1"), ((2, 3, 5), "1")):
        got, _ = fields(tool, case("lds", "BAXT", mode, **kw))
        assert got["waves_per_workgroup"] == waves, (mode, got)
    # ... and a shorter pair keeps its four waves under a table
    got, _ = fields(tool, case("lds/short", "BAXT", (2, 3, 5), env={"DPX_WPB": 4}, m=19000, pairs=1, band=16))
    assert got["waves_per_workgroup"] == "4", got
    # the plan itself is the same whatever the mode
    states = {fields(tool, case("lds", "BAXT", mode, **kw))[0]["state"] for mode in ((-1, -1, 0), (2, 3, 5))}
    assert len(states) == 1
