"""Which kernels a batch runs (csrc/dpx_plan.cpp: dpx_plan_route) on the CPU, through hostcpp/plan_tool with a `mode` line: the fill
kernel and the traceback that dpx_batch_describe() names, and the walk family and mode that the traceback launches.

The expectations below were written by hand from the if-chains of the commit before the route existed -- launch_main and launch_all
(fill), traceback_lines (walk family; walk mode with its 20 000- and 65 536-pair thresholds and DPX_TB_WALK) in csrc/dpx_capi.cpp (today: dpx_capi.cpp and dpx_output.cpp's lines_behind_fill) -- and
from the planner's own rules for lanes, couples and the split kernel.  None of them was produced by running the code under test.
A direction or band-direction batch has one walk and takes no mode: the route says 0 whatever the knob says.

Every pair is 8 x 8 (so 65 536 pairs are only a pair table), except the split kernel's: it needs two stripes, a query over 128 rows."""
import pytest

import plan_cases
import test_batch_plan

W = [3, -1, -2, -1]
DIRS, BAND_DIRS = 8, 16
POST_CREATION = {"k_zext_fill", "k_subst_fill", "k_zsub_fill"}


def case(name, algo, kernel, walk, traceback=None, band=0, flags=0, env=None, mode=(-1, -1, 0), pairs=4, m=8):
    return {"name": name, "algo": algo, "weights": W, "band": band, "flags": flags, "env": env or {}, "gen": ["make_batch", pairs, m, 8, 1],
            "mode": list(mode), "kernel": kernel, "traceback": traceback, "walk": walk}


ROUTES = [
    # the fill kernels a batch gets at its creation
    case("linear/fill", "LSW", "k_linear_fill", "plain:2"),
    case("linear/fill/LNW", "LNW", "k_linear_fill", "plain:2"),
    case("linear/fill_pk", "LSW", "k_linear_fill_pk", "plain:2", env={"DPX_PACKED": 1}),
    case("linear/lanes", "LSW", "k_linear_lanes", "plain:2", env={"DPX_LANES": 1, "DPX_LANES_PK": 0}),
    case("linear/lanes_pk", "LSW", "k_linear_lanes_pk", "plain:2", env={"DPX_LANES": 1}),
    case("linear/split", "LSW", "k_linear_split", "plain:2", m=200),
    case("affine/fill", "ANW", "k_affine_fill", "plain:2"),
    case("affine/asw_fill", "ASW", "k_asw_fill", "plain:2"),
    case("affine/asg_fill", "ASG", "k_asg_fill", "plain:2"),
    case("affine/lanes", "ANW", "k_affine_lanes", "plain:2", env={"DPX_LANES": 1}),
    case("affine/asw_lanes", "ASW", "k_asw_lanes", "plain:2", env={"DPX_LANES": 1}),
    case("affine/asg_lanes", "ASG", "k_asg_lanes", "plain:2", env={"DPX_LANES": 1}),
    case("band/bsw", "BSW", "k_banded_fill", "plain:2", band=4),
    case("band/bsw_pk", "BSW", "k_banded_fill_pk", "plain:2", band=4, env={"DPX_PACKED": 1}),
    case("band/basw", "BASW", "k_basw_fill", "basw:2", "k_basw_traceback_wave", band=4),
    case("band/banw", "BANW", "k_banw_fill", "banw:2", "k_banw_traceback_wave", band=4),
    case("band/baxt", "BAXT", "k_baxt_fill", "banw:2", "k_banw_traceback_wave", band=4),
    case("banddir/banw", "BANW", "k_bdir_fill", "bdir:0", "k_bdir_traceback", band=4, flags=BAND_DIRS),
    case("banddir/baxt", "BAXT", "k_bdir_fill", "bdir:0", "k_bdir_traceback", band=4, flags=BAND_DIRS),
    case("dir/lsw", "LSW", "k_linear_dir", "dir:0", flags=DIRS),
    case("dir/lnw", "LNW", "k_linear_dir", "dir:0", flags=DIRS),
    case("dir/anw", "ANW", "k_affine_dir", "dir:0", flags=DIRS),
    case("dir/asw", "ASW", "k_asw_dir", "dir:0", flags=DIRS),
    case("dir/asg", "ASG", "k_asg_dir", "dir:0", flags=DIRS),
    # a band that covers the matrix runs the unbanded kernel, its walk included (BANW: band >= 9, its band applies to the borders too)
    case("covering/bsw", "BSW", "k_linear_fill", "plain:2", band=8),
    case("covering/basw", "BASW", "k_asw_fill", "plain:2", band=8),
    case("covering/banw", "BANW", "k_affine_fill", "plain:2", band=9),
    case("covering/banw/band_dirs", "BANW", "k_affine_dir", "dir:0", band=9, flags=BAND_DIRS),
    # what a batch can change after its creation
    case("mode/zext", "BAXT", "k_zext_fill", "banw:2", "k_banw_traceback_wave", band=4, mode=(2, -1, 0)),
    case("mode/zext/bonus_only", "BAXT", "k_zext_fill", "banw:2", "k_banw_traceback_wave", band=4, mode=(-1, 3, 0)),
    case("mode/subst/banw", "BANW", "k_subst_fill", "subst:2", "k_subst_traceback_wave", band=4, mode=(-1, -1, 5)),
    case("mode/subst/baxt", "BAXT", "k_subst_fill", "subst:2", "k_subst_traceback_wave", band=4, mode=(-1, -1, 5)),
    case("mode/zsub", "BAXT", "k_zsub_fill", "subst:2", "k_subst_traceback_wave", band=4, mode=(2, 3, 5)),
    case("mode/zsub/bonus_only", "BAXT", "k_zsub_fill", "subst:2", "k_subst_traceback_wave", band=4, mode=(-1, 3, 5)),
]

# walk mode with DPX_TB_WALK unset: linear gaps always the wave walk; three planes the wave walk up to 20 000 pairs, then one lane per
# pair cell by cell, from 65 536 pairs on through cached column vectors.  (From 4096 pairs on the 8 x 8 LSW batch runs in couples:
# twelve one-lane pairs would fill a fifth of a lane-packed wave, under the 85 % that path asks for.)
for pairs, three_planes in ((20000, 2), (20001, 0), (65535, 0), (65536, 1)):
    wave = "_wave" if three_planes == 2 else ""
    ROUTES += [
        case(f"walk/lsw/{pairs}", "LSW", "k_linear_fill_pk", "plain:2", pairs=pairs),
        case(f"walk/anw/{pairs}", "ANW", "k_affine_fill", f"plain:{three_planes}", pairs=pairs),
        case(f"walk/asw/{pairs}", "ASW", "k_asw_fill", f"plain:{three_planes}", pairs=pairs),
        case(f"walk/basw/{pairs}", "BASW", "k_basw_fill", f"basw:{three_planes}", "k_basw_traceback" + wave, band=4, pairs=pairs),
        case(f"walk/banw/{pairs}", "BANW", "k_banw_fill", f"banw:{three_planes}", "k_banw_traceback" + wave, band=4, pairs=pairs),
        case(f"walk/baxt_table/{pairs}", "BAXT", "k_subst_fill", f"subst:{three_planes}", "k_subst_traceback" + wave, band=4, pairs=pairs,
             mode=(-1, -1, 5)),
    ]
ROUTES += [case("walk/bsw/small", "BSW", "k_banded_fill", "plain:2", band=4)]

# DPX_TB_WALK forces a walk, min(2, value); batches with one walk ignore it
for knob in (0, 1, 2, 3):
    mode = min(knob, 2)
    wave = "_wave" if mode == 2 else ""
    env = {"DPX_TB_WALK": knob}
    ROUTES += [
        case(f"knob{knob}/lsw", "LSW", "k_linear_fill", f"plain:{mode}", env=env),
        case(f"knob{knob}/anw", "ANW", "k_affine_fill", f"plain:{mode}", env=env),
        case(f"knob{knob}/basw", "BASW", "k_basw_fill", f"basw:{mode}", "k_basw_traceback" + wave, band=4, env=env),
        case(f"knob{knob}/banw", "BANW", "k_banw_fill", f"banw:{mode}", "k_banw_traceback" + wave, band=4, env=env),
        case(f"knob{knob}/zsub", "BAXT", "k_zsub_fill", f"subst:{mode}", "k_subst_traceback" + wave, band=4, env=env, mode=(2, 3, 5)),
        case(f"knob{knob}/dir", "LSW", "k_linear_dir", "dir:0", flags=DIRS, env=env),
        case(f"knob{knob}/banddir", "BAXT", "k_bdir_fill", "bdir:0", "k_bdir_traceback", band=4, flags=BAND_DIRS, env=env),
    ]


@pytest.fixture(scope="module")
def tool():
    return plan_cases.build_tool()


@pytest.fixture(scope="module")
def printed(tool):
    """plan_tool's fields for a case, each case run once"""
    seen = {}

    def get(c):
        if c["name"] not in seen:
            line = plan_cases.run_tool(tool, c)
            assert line.startswith("status=0 "), line
            seen[c["name"]] = dict(kv.split("=", 1) for kv in line.split()[1:])
        return seen[c["name"]]

    return get


@pytest.mark.parametrize("c", ROUTES, ids=[c["name"] for c in ROUTES])
def test_route(printed, c):
    got = printed(c)
    assert (got["kernel"], got.get("traceback"), got["walk"]) == (c["kernel"], c["traceback"], c["walk"]), got
    z, e, alphabet = c["mode"]
    extension = c["algo"] == "BAXT" and (z >= 0 or e >= 0)
    assert (got.get("zdrop"), got.get("end_bonus")) == ((str(z), str(e)) if extension else (None, None)), got
    assert got.get("subst") == (str(alphabet) if alphabet else None), got


def test_no_mode_line_no_walk_field(tool):
    c = dict(ROUTES[0])
    del c["mode"]
    assert " walk=" not in plan_cases.run_tool(tool, c)


def test_every_fill_kernel_is_seen_under_its_own_name(printed):
    """24 enumerators, 24 different names: the create-time ones of the golden plans and the three a setter brings"""
    names = {printed(c)["kernel"] for c in ROUTES}
    assert names == test_batch_plan.KERNELS | POST_CREATION and len(names) == 24
