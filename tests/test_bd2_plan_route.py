"""What a DPX_TWO_PIECE_GAPS batch runs (csrc/dpx_plan.cpp), on the CPU through hostcpp/plan_tool: the flag gives k_bd2_fill /
k_bd2_traceback / bd2:0 / banddir8 in every mode, the pool is sized by the byte layout (ceil((m + n - 1) / (16 / C)) chunks of 1 KiB), a
band of 257 is unsupported and a covering BANW band stays on the band kernel, 0x20 without 0x10 is invalid, the mode fields keep their
order with ` gap2=` behind the layout, and the unflagged plan is what it was."""
import subprocess

import pytest

import plan_cases

W = [3, -1, -2, -1]
BAND_DIRS, TWO_PIECE = 16, 32
INVALID, UNSUPPORTED = -1, -8
MODES = [(-1, -1, 0), (-1, -1, 5), (-1, 3, 0), (2, 3, 0), (-1, 3, 5), (2, 3, 5)]


def case(name, algo, mode=None, m=8, n=None, pairs=4, flags=BAND_DIRS | TWO_PIECE, band=4, env=None):
    c = {"name": name, "algo": algo, "weights": W, "band": band, "flags": flags, "env": env or {}, "gen": ["make_batch", pairs, m, n or m, 1]}
    if mode is not None:
        c["mode"] = list(mode)
    return c


@pytest.fixture(scope="module")
def tool():
    return plan_cases.build_tool()


def run(tool, c, gap2=None):
    text = plan_cases.tool_input(c, plan_cases.make_input(c))
    if gap2 is not None:  # the optional line for the second piece: behind the header (and the mode line), before the pairs
        lines = text.split("\n")
        at = 5 if "mode" in c else 4
        text = "\n".join(lines[:at] + ["gap2 %d %d" % gap2] + lines[at:])
    r = subprocess.run([tool], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (c["name"], r.stderr[-2000:])
    return r.stdout.rstrip("\n")


def fields(tool, c, gap2=None):
    line = run(tool, c, gap2)
    assert line.startswith("status=0 "), line
    return dict(kv.split("=", 1) for kv in line.split()[1:]), line


@pytest.mark.parametrize("algo,mode", [("BANW", MODES[0]), ("BANW", MODES[1])] + [("BAXT", m) for m in MODES])
def test_the_flag_runs_the_two_piece_kernels_in_every_mode(tool, algo, mode):
    got, line = fields(tool, case("bd2", algo, mode), gap2=(-24, -1))
    assert (got["kernel"], got["traceback"], got["walk"], got["matrix"], got["gap2"]) == ("k_bd2_fill", "k_bd2_traceback", "bd2:0", "banddir8", "-24,-1"), got
    z, e, alphabet = mode
    tail = line[line.index(" traceback="):line.index(" info=")]
    want = " traceback=k_bd2_traceback" + (f" zdrop={z} end_bonus={e}" if (z >= 0 or e >= 0) else "") + (f" subst={alphabet}" if alphabet else "")
    assert tail == want + " matrix=banddir8 gap2=-24,-1", tail
    assert fields(tool, case("bd2", algo, mode))[0]["gap2"] == "-2,-1"  # until the setter is called: piece 1
    assert fields(tool, case("bd2", algo, mode, env={"DPX_TB_WALK": 2}))[0]["walk"] == "bd2:0"  # one walk


@pytest.mark.parametrize("band,cpl", [(1, 1), (64, 1), (65, 2), (128, 2), (129, 4), (256, 4)])
def test_the_pool_is_sized_by_the_byte_layout(tool, band, cpl):
    m, n = 300, 321
    got, _ = fields(tool, case("chunks", "BAXT", MODES[0], m=m, n=n, pairs=3, band=band))
    gd = 16 // cpl
    chunks = -(-(m + n - 1) // gd)
    assert got["rows_per_lane"] == str(cpl)
    assert int(got["info"].split(",")[2]) == 3 * chunks * 1024, (got["info"], chunks)
    plain, _ = fields(tool, case("chunks", "BAXT", MODES[0], m=m, n=n, pairs=3, band=band, flags=BAND_DIRS))
    assert int(plain["info"].split(",")[2]) == 3 * -(-(m + n - 1) // (2 * gd)) * 1024  # twice k_bdir_fill's bytes


def test_refusals(tool):
    assert run(tool, case("wide", "BAXT", band=257)).startswith("status=%d" % UNSUPPORTED)
    assert run(tool, case("wide", "BANW", band=257, m=20)).startswith("status=%d" % UNSUPPORTED)  # covering or not
    assert run(tool, case("wide", "BAXT", band=512, flags=BAND_DIRS)).startswith("status=0 ")  # (the unflagged batch goes to 512)
    for algo in ("BAXT", "BANW", "LSW"):
        assert run(tool, case("alone", algo, flags=TWO_PIECE)).startswith("status=%d" % INVALID), algo  # 0x20 without 0x10
    for algo in ("LSW", "ANW", "BSW", "BASW"):
        assert run(tool, case("algo", algo)).startswith("status=%d" % UNSUPPORTED), algo


def test_a_covering_banw_band_stays_on_the_band_kernel(tool):
    got, _ = fields(tool, case("cover", "BANW", MODES[0], m=20, band=21))
    assert (got["kernel_algo"], got["kernel"], got["matrix"]) == ("BANW", "k_bd2_fill", "banddir8"), got
    plain, _ = fields(tool, case("cover", "BANW", MODES[0], m=20, band=21, flags=BAND_DIRS))
    assert (plain["kernel_algo"], plain["kernel"], plain["matrix"]) == ("ANW", "k_affine_dir", "dir4"), plain


@pytest.mark.parametrize("algo", ["BANW", "BAXT"])
def test_the_unflagged_plan_is_unchanged(tool, algo):
    got, line = fields(tool, case("plain", algo, MODES[0], flags=BAND_DIRS), gap2=(-24, -1))  # (a gap2 line without the flag: ignored)
    assert (got["kernel"], got["traceback"], got["walk"], got["matrix"]) == ("k_bdir_fill", "k_bdir_traceback", "bdir:0", "banddir4"), got
    assert "gap2" not in got and line == run(tool, case("plain", algo, MODES[0], flags=BAND_DIRS))
