"""What an ANW / ASW / ASG direction batch runs under dpx_batch_set_direction_table (csrc/dpx_plan.cpp: dpx_plan_route,
dpx_plan_dirtab_waves), on the CPU through hostcpp/plan_tool with a `mode` line: the table is a mode of the three kernel= names with
the one walk of direction batches, ` subst=` is printed as the other table modes print it, and the workgroup shrinks to one wave exactly
when the plan's waves fit one workgroup's LDS without the 1280-byte table image and not with it."""
import pytest

import plan_cases

W = [3, -1, -2, -1]
KEEP_DIRECTIONS = 8
LDS_MAX, IMAGE = 160 * 1024, 1280  # one workgroup's LDS; DPX_SUBST_IMAGE_BYTES per wave
KERNEL = {"ANW": "k_affine_dir", "ASW": "k_asw_dir", "ASG": "k_asg_dir"}


def case(name, algo, alphabet, env=None, m=8, n=8, pairs=4):
    return {"name": name, "algo": algo, "weights": W, "band": 0, "flags": KEEP_DIRECTIONS, "env": env or {}, "gen": ["make_batch", pairs, m, n, 1],
            "mode": [-1, -1, alphabet]}


def dir_per_wave(n):
    """main_lds (dpx_plan.cpp): two int32 edge rows of n + 2 and the staged reference of n + 192 bytes, each rounded up to 16"""
    return 2 * (-(-((n + 2) * 4) // 16) * 16) + -(-(n + 192) // 16) * 16


@pytest.fixture(scope="module")
def tool():
    return plan_cases.build_tool()


def fields(tool, c):
    line = plan_cases.run_tool(tool, c)
    assert line.startswith("status=0 "), line
    return dict(kv.split("=", 1) for kv in line.split()[1:]), line


@pytest.mark.parametrize("algo", sorted(KERNEL))
def test_the_table_is_a_mode_of_the_same_route(tool, algo):
    plain, pline = fields(tool, case("plain", algo, 0))
    got, line = fields(tool, case("table", algo, 24))
    assert (got["kernel"], got["walk"], got["matrix"], got["dir_edges"], got["subst"]) == (KERNEL[algo], "dir:0", "dir4", "lds", "24"), got
    assert "subst" not in plain and (plain["kernel"], plain["walk"]) == (KERNEL[algo], "dir:0")
    assert line.replace(" subst=24", "") == pline and " subst=24 matrix=dir4 " in line  # nothing else moves; printed before the batch's own matrix=
    assert got["state"] == plain["state"]  # the plan itself is the same


def test_the_workgroup_shrinks_only_when_the_images_do_not_fit(tool):
    n = 4480  # between the two four-wave thresholds
    assert 4 * dir_per_wave(n) <= LDS_MAX < 4 * (dir_per_wave(n) + IMAGE)
    lo = next(x for x in range(4000, 5000) if 4 * (dir_per_wave(x) + IMAGE) > LDS_MAX)
    hi = next(x for x in range(4000, 5000) if 4 * dir_per_wave(x) > LDS_MAX)
    assert 4300 < lo <= n < hi < 4600
    for algo in sorted(KERNEL):
        for length, alphabet, waves in ((n, 0, "4"), (n, 5, "1"), (lo - 1, 5, "4"), (lo, 5, "1"), (hi, 0, "1"), (hi, 5, "1"), (300, 32, "4")):
            got, _ = fields(tool, case("lds", algo, alphabet, env={"DPX_WPB": 4}, m=70, n=length, pairs=1))
            assert got["waves_per_workgroup"] == waves and got["dir_edges"] == "lds", (algo, length, alphabet, got)
    # edge rows in global memory: one wave per workgroup with or without the table, which then is all the LDS holds
    far = next(x for x in range(7000, 8000) if dir_per_wave(x) > 64 * 1024)
    assert 7200 < far < 7300
    for alphabet in (0, 5):
        got, _ = fields(tool, case("global", "ASW", alphabet, env={"DPX_R": 2}, m=130, n=far, pairs=1))
        assert (got["waves_per_workgroup"], got["dir_edges"], got["rows_per_lane"]) == ("1", "global", "2"), got
