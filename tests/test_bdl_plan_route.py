"""What a DPX_KEEP_LOCAL_BAND_DIRECTIONS batch of BSW / BASW runs (csrc/dpx_plan.cpp), on the CPU through hostcpp/plan_tool: the flag gives
k_bdl_fill / k_bdl_traceback / bdl:0 / banddir4 with int32 arithmetic and C cells per lane, the pool is sized by the nibble layout
(ceil((m + n - 1) / (32 / C)) chunks of 1 KiB), a covering band takes the matrix batch's fall-back as an LSW / ASW direction batch, every
refusal of the flag's list answers its status, pairs the int16 batch refuses with DPX_ERR_RANGE are planned, and the plan without the
flag is what it was."""
import subprocess

import pytest

import plan_cases

W = [3, -1, -2, -1]
SCORE_ONLY, DIRS, BAND_DIRS, TWO_PIECE, LOCAL = 1, 8, 16, 32, 64
INVALID, RANGE, UNSUPPORTED = -1, -4, -8
NO_MODE = (-1, -1, 0)


def case(name, algo, m=300, n=None, pairs=4, flags=LOCAL, band=4, env=None, mode=NO_MODE):
    c = {"name": name, "algo": algo, "weights": W, "band": band, "flags": flags, "env": env or {}, "gen": ["make_batch", pairs, m, n or m, 1]}
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


@pytest.mark.parametrize("algo", ["BSW", "BASW"])
def test_the_flag_runs_the_local_band_direction_kernels(tool, algo):
    got, line = fields(tool, case("bdl", algo))
    assert (got["algo"], got["kernel_algo"], got["kernel"], got["traceback"], got["walk"], got["matrix"]) == \
        (algo, algo, "k_bdl_fill", "k_bdl_traceback", "bdl:0", "banddir4"), got
    assert (got["dtype"], got["rows_per_lane"], got["store"], got["couples"], got["lane_pairs"]) == ("int32", "1", "1", "0", "0"), got
    assert line[line.index(" traceback="):line.index(" info=")] == " traceback=k_bdl_traceback matrix=banddir4", line
    for walk in (0, 1, 2):  # one walk: DPX_TB_WALK has no effect
        assert fields(tool, case("bdl", algo, env={"DPX_TB_WALK": walk}))[0]["walk"] == "bdl:0"
    # a batch large enough for the packed-int16 couples of BSW stays on the one kernel
    big, _ = fields(tool, case("bdl", algo, m=64, pairs=5000, band=8))
    assert (big["kernel"], big["couples"], big["dtype"]) == ("k_bdl_fill", "0", "int32"), big


@pytest.mark.parametrize("algo", ["BSW", "BASW"])
@pytest.mark.parametrize("band,cpl", [(1, 1), (64, 1), (65, 2), (128, 2), (129, 4), (256, 4), (257, 8), (512, 8)])
def test_the_pool_is_sized_by_the_nibble_layout(tool, algo, band, cpl):
    m, n = 600, 641
    got, _ = fields(tool, case("chunks", algo, m=m, n=n, pairs=3, band=band))
    chunks = -(-(m + n - 1) // (32 // cpl))
    assert got["rows_per_lane"] == str(cpl)
    assert int(got["info"].split(",")[2]) == 3 * chunks * 1024, (got["info"], chunks)


@pytest.mark.parametrize("algo,kalgo", [("BSW", "LSW"), ("BASW", "ASW")])
def test_a_covering_band_runs_as_a_direction_batch_of_the_unbanded_algorithm(tool, algo, kalgo):
    got, _ = fields(tool, case("cover", algo, m=20, band=20))
    plain, _ = fields(tool, case("cover", kalgo, m=20, band=0, flags=DIRS))  # what an LSW / ASW direction batch runs
    assert got["kernel_algo"] == kalgo and got["matrix"] == "dir4" and got["kernel"] == plain["kernel"], (got, plain)
    assert got["kernel"] in ("k_linear_dir", "k_asw_dir") and got["walk"] == "dir:0", got
    for key in ("dtype", "rows_per_lane", "waves_per_workgroup", "dir_edges", "dir_scratch_bytes"):
        assert got[key] == plain[key], key
    assert fields(tool, case("cover", algo, m=20, band=600))[0]["matrix"] == "dir4"  # wider than 512, and covering: admitted
    assert fields(tool, case("cover", algo, m=20, band=19))[0]["kernel"] == "k_bdl_fill"  # one short of covering


def test_statuses(tool):
    for algo in ("BSW", "BASW"):
        for extra in (SCORE_ONLY, BAND_DIRS, TWO_PIECE, BAND_DIRS | TWO_PIECE):
            assert status(tool, case("with", algo, flags=LOCAL | extra)) == INVALID, (algo, extra)
        assert status(tool, case("with8", algo, flags=LOCAL | DIRS)) == UNSUPPORTED, algo
        assert status(tool, case("wide", algo, band=513, m=600)) == UNSUPPORTED, algo  # band > 512 and not covering
        assert status(tool, case("wide", algo, band=512, m=600)) == 0, algo
    for algo in ("LNW", "LSW", "ANW", "ASW", "ASG", "BANW", "BAXT"):
        assert status(tool, case("algo", algo, band=8, m=10)) == UNSUPPORTED, algo
    # strings that do not fit LDS: one-wave workgroups first, then refused
    four, _ = fields(tool, case("lds", "BASW", m=30000, pairs=2, band=64))
    assert four["waves_per_workgroup"] == "1", four
    assert status(tool, case("lds", "BASW", m=90000, pairs=1, band=64)) == UNSUPPORTED


@pytest.mark.parametrize("algo", ["BSW", "BASW"])
def test_pairs_the_int16_batch_refuses_are_planned(tool, algo):
    assert status(tool, case("long", algo, m=33000, pairs=1, band=64, flags=0)) == RANGE
    got, _ = fields(tool, case("long", algo, m=33000, pairs=1, band=64))
    assert got["kernel"] == "k_bdl_fill" and int(got["info"].split(",")[2]) == -(-(2 * 33000 - 1) // 32) * 1024, got
    assert status(tool, case("past", algo, m=8, pairs=1, band=2, mode=None) | {"weights": [1 << 20, -1, -2, -1], "gen": ["make_batch", 1, 300, 300, 1]}) == RANGE  # 2^20 * 300 > 2^28


@pytest.mark.parametrize("algo,kernel", [("BSW", "k_banded_fill"), ("BASW", "k_basw_fill")])
def test_the_plan_without_the_flag_is_unchanged(tool, algo, kernel):
    got, line = fields(tool, case("plain", algo, flags=0))
    assert got["kernel"] == kernel and "matrix" not in got and got["walk"] == ("plain:2" if algo == "BSW" else "basw:2"), got
    assert ("traceback" in got) == (algo == "BASW")
