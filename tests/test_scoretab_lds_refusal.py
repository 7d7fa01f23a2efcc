"""dpx_batch_set_score_table's refusal for LDS (DPX_ERR_UNSUPPORTED with text in dpx_last_error()), on the CPU.  Creation admits an ANW /
ASW / ASG score-only batch only when FOUR plain slices of its longest reference fit one workgroup's 160 KiB (launch_scalars, lane-packed
plans included), so one slice plus the 1280-byte image always fits a batch that exists: the first test shows that through plan_tool at
the longest reference creation admits.  The second drives dpx_plan_scoretab_waves / dpx_plan_scoretab_fits, which the setter calls,
past that limit on hand-made plans (tests/scoretab_fits_main.cpp beside csrc/dpx_plan.cpp) and checks both messages."""
import os
import shutil
import subprocess

import pytest

import plan_cases
from test_scoretab_plan_route import IMAGE, LDS_MAX, case, per_wave

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "csrc")


def test_no_batch_that_creation_admits_reaches_the_refusal():
    tool = plan_cases.build_tool()
    for m in (1, 70, 512):
        hi = next(x for x in range(5000, 9000) if 4 * per_wave(x, m) > LDS_MAX)  # the first reference length creation refuses
        assert per_wave(hi - 1, m) + IMAGE <= LDS_MAX // 3  # one slice with its image: a third of a workgroup's LDS at the most
        for lanes in (0, 1):
            env = {"DPX_LANES": lanes, "DPX_WPB": 4}
            assert plan_cases.run_tool(tool, case("over", "ASW", 5, env, m=m, n=hi, pairs=1)).startswith("status=-8")
            line = plan_cases.run_tool(tool, case("edge", "ASW", 5, env, m=m, n=hi - 1, pairs=1))
            assert line.startswith("status=0 ") and " subst=5" in line and " waves_per_workgroup=1 " in line, line


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path_factory.mktemp("scoretab_fits") / "scoretab_fits")
    subprocess.run([cxx, "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", inc, "-o", exe, os.path.join(ROOT, "tests", "scoretab_fits_main.cpp"),
                    os.path.join(CSRC, "dpx_plan.cpp")], check=True)
    return exe


def _ask(exe, *rows):
    out = subprocess.run([exe], input="".join(" ".join(map(str, r)) + "\n" for r in rows), capture_output=True, text=True, check=True).stdout
    return [dict(kv.split("=", 1) for kv in line.split(" ", 2)) for line in out.splitlines()]


def test_the_helpers_refuse_past_the_limit_with_text(harness):
    fit = LDS_MAX - IMAGE  # the largest slice that fits with its image
    rows = [(LDS_MAX // 4 - IMAGE, 4, 5, 0, 0), (LDS_MAX // 4 - IMAGE + 16, 4, 5, 0, 0), (fit, 4, 5, 0, 0), (fit + 16, 4, 5, 0, 0), (fit + 16, 1, 5, 0, 0),
            (1024, 4, 0, 1, fit), (1024, 4, 0, 1, fit + 16), (fit + 16, 4, 0, 1, 2048), (fit + 16, 4, 3, 1, 2048)]
    got = _ask(harness, *rows)
    assert [(g["waves"], g["fits"]) for g in got] == [("4", "1"), ("1", "1"), ("1", "1"), ("0", "0"), ("0", "0"),
                                                     ("4", "1"), ("4", "0"), ("0", "1"), ("0", "0")]
    for k in (3, 4, 8):  # one wave's slice with the image: the sizes are named
        assert got[k]["err"] == f"score table: one wave's LDS slice with the table image ({fit + 16 + IMAGE} bytes) exceeds a workgroup's {LDS_MAX}", got[k]
    assert got[6]["err"] == f"score table: a lane-packed wave's LDS with the table image ({fit + 16 + IMAGE} bytes) exceeds a workgroup's {LDS_MAX}", got[6]
    assert all(g["err"] == "" for g in got if g["fits"] == "1")
