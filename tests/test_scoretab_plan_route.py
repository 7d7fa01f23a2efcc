"""What an ANW / ASW / ASG score-only batch runs under dpx_batch_set_score_table (csrc/dpx_plan.cpp: dpx_plan_route,
dpx_plan_scoretab_waves), on the CPU through hostcpp/plan_tool with a `mode` line: the table is a mode of the six kernel= names (the plan
itself, its state= and every other field stay), ` subst=` is printed as the other table modes print it, the one-wave-per-pair fill's
workgroup shrinks to one wave exactly when four slices fit one workgroup's LDS without the 1280-byte table images and not with them,
and the lines of the table modes that existed before (BANW / BAXT) are what they were."""
import pytest

import plan_cases

W = [3, -1, -4, -1]
SCORE_ONLY = 1
LDS_MAX, IMAGE = 160 * 1024, 1280  # one workgroup's LDS; DPX_SUBST_IMAGE_BYTES per wave
FILL = {"ANW": "k_affine_fill", "ASW": "k_asw_fill", "ASG": "k_asg_fill"}
LANES = {"ANW": "k_affine_lanes", "ASW": "k_asw_lanes", "ASG": "k_asg_lanes"}


def case(name, algo, alphabet, env=None, m=300, n=300, pairs=8, flags=SCORE_ONLY, band=0):
    return {"name": name, "algo": algo, "weights": W, "band": band, "flags": flags, "env": env or {}, "gen": ["make_batch", pairs, m, n, 1],
            "mode": [-1, -1, alphabet]}


def _up(v):
    return -(-v // 16) * 16


def per_wave(n, m):
    """main_lds (dpx_plan.cpp): two int16 edge rows of n + 2, the staged reference of n + 144 bytes and the staged query of the rolling
    schedule, m + 1056 bytes, each rounded up to 16"""
    return 2 * _up((n + 2) * 2) + _up(n + 144) + _up(m + 1056)


@pytest.fixture(scope="module")
def tool():
    return plan_cases.build_tool()


def fields(tool, c):
    line = plan_cases.run_tool(tool, c)
    assert line.startswith("status=0 "), line
    return dict(kv.split("=", 1) for kv in line.split()[1:]), line


@pytest.mark.parametrize("algo", sorted(FILL))
@pytest.mark.parametrize("lanes", [0, 1])
def test_the_table_is_a_mode_of_the_same_route(tool, algo, lanes):
    env = {"DPX_LANES": lanes, "DPX_WPB": 4}  # (a small launch would take one-wave workgroups by itself)
    shape = dict(m=40, n=120, pairs=40) if lanes else dict(m=300, n=300, pairs=8)
    plain, pline = fields(tool, case("plain", algo, 0, env, **shape))
    got, line = fields(tool, case("table", algo, 24, env, **shape))
    kernel = (LANES if lanes else FILL)[algo]
    assert (got["kernel"], got["store"], got["subst"]) == (kernel, "0", "24"), got
    assert "subst" not in plain and (plain["kernel"], plain["store"]) == (kernel, "0"), plain
    assert line.replace(" subst=24", "") == pline  # nothing else moves: waves, state, walk
    assert got["state"] == plain["state"]  # the plan itself is the same
    assert (int(got["waves"]) > 0) == bool(lanes) and got["waves_per_workgroup"] == ("1" if lanes else "4")


def test_the_workgroup_shrinks_only_when_the_images_do_not_fit(tool):
    m = 70
    lo = next(x for x in range(5000, 9000) if 4 * (per_wave(x, m) + IMAGE) > LDS_MAX)  # the first reference length whose four slices do not fit with the images
    hi = next(x for x in range(5000, 9000) if 4 * per_wave(x, m) > LDS_MAX)            # ... nor without them: the plain batch is refused from here on
    assert 7000 < lo < hi < 8000 and 4 * per_wave(lo - 1, m) <= LDS_MAX
    for algo in sorted(FILL):
        for length, alphabet, waves in ((lo - 1, 0, "4"), (lo - 1, 5, "4"), (lo, 0, "4"), (lo, 5, "1"), (hi - 1, 0, "4"), (hi - 1, 5, "1"), (300, 32, "4")):
            got, _ = fields(tool, case("lds", algo, alphabet, env={"DPX_WPB": 4, "DPX_LANES": 0}, m=m, n=length, pairs=1))
            assert got["waves_per_workgroup"] == waves and got["kernel"] == FILL[algo], (algo, length, alphabet, got)
        line = plan_cases.run_tool(tool, case("lds", algo, 0, env={"DPX_WPB": 4, "DPX_LANES": 0}, m=m, n=hi, pairs=1))
        assert line.startswith("status=-8"), line  # (DPX_ERR_UNSUPPORTED: four plain slices no longer fit)
    got, _ = fields(tool, case("one", "ASW", 5, env={"DPX_WPB": 1, "DPX_LANES": 0}, m=m, n=lo, pairs=1))
    assert got["waves_per_workgroup"] == "1"


# plan_tool's lines for the table modes of BANW / BAXT matrix batches, recorded on the commit before the score-only route existed
BEFORE = {
    ("BANW", 0): "status=0 algo=BANW kernel_algo=BANW kernel=k_banw_fill dtype=int32 rows_per_lane=1 store=1 couples=0 lane_pairs=0 waves=0 singles=6 row_tags=0 seq_input=bytes waves_per_workgroup=1 traceback=k_banw_traceback_wave info=6,264000,976896,436056 state=bb7f31cd68538efe walk=banw:2",
    ("BANW", 24): "status=0 algo=BANW kernel_algo=BANW kernel=k_subst_fill dtype=int32 rows_per_lane=1 store=1 couples=0 lane_pairs=0 waves=0 singles=6 row_tags=0 seq_input=bytes waves_per_workgroup=1 traceback=k_subst_traceback_wave subst=24 info=6,264000,976896,436056 state=bb7f31cd68538efe walk=subst:2",
    ("BAXT", 0): "status=0 algo=BAXT kernel_algo=BAXT kernel=k_baxt_fill dtype=int32 rows_per_lane=1 store=1 couples=0 lane_pairs=0 waves=0 singles=6 row_tags=0 seq_input=bytes waves_per_workgroup=1 traceback=k_banw_traceback_wave info=6,264000,976896,436056 state=4670f058a23ac3d3 walk=banw:2",
    ("BAXT", 24): "status=0 algo=BAXT kernel_algo=BAXT kernel=k_subst_fill dtype=int32 rows_per_lane=1 store=1 couples=0 lane_pairs=0 waves=0 singles=6 row_tags=0 seq_input=bytes waves_per_workgroup=1 traceback=k_subst_traceback_wave subst=24 info=6,264000,976896,436056 state=4670f058a23ac3d3 walk=subst:2",
}


@pytest.mark.parametrize("key", sorted(BEFORE))
def test_the_older_table_modes_print_what_they_printed(tool, key):
    algo, alphabet = key
    line = plan_cases.run_tool(tool, case("band", algo, alphabet, m=200, n=220, pairs=6, flags=0, band=32))
    assert line == BEFORE[key]
    assert ("kernel=k_subst_fill" in line and " subst=24" in line and "walk=subst:" in line) == bool(alphabet)
