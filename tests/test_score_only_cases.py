"""tests/score_only_cases.py without a GPU: what tests/test_gpu_score_only.py relies on holds on the oracles and on the planner alone --
pairs of two or more stripes over 128 or more columns exist in every parametrization, the crafted ties lie in different stripes, the
band changes an answer, and the planner sends every case where the GPU test asserts it ran (plan_tool, csrc/dpx_plan.cpp)."""
import subprocess

import pytest

import plan_cases
import score_only_cases as S

SCORE_ONLY = 1


@pytest.fixture(scope="module")
def oracles(tmp_path_factory):
    return S.build_oracles(tmp_path_factory.mktemp("score_only_oracles"))


@pytest.fixture(scope="module")
def tool():
    return plan_cases.build_tool()


def _plan(tool, algo, sb, env, band=0, flags=SCORE_ONLY):
    case = {"name": "score-only", "algo": algo, "weights": list(S.W[algo]), "band": band, "flags": flags, "env": env}
    r = subprocess.run([tool], input=plan_cases.tool_input(case, sb), capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    fields = dict(kv.split("=", 1) for kv in r.stdout.split() if "=" in kv)
    assert fields["status"] == "0", r.stdout
    return fields


def _is(fields, **want):
    assert {k: fields[k] for k in want} == {k: str(v) for k, v in want.items()}, fields


@pytest.mark.parametrize("algo,R", S.STRIPED)
def test_striped_cases_reach_the_striped_loop(tool, algo, R):
    sb = S.striped_batch(R)   # (striped_shapes asserts that pairs with S >= 2 and n >= 128 exist)
    reached = [p for p in range(sb.num_pairs) if S.stripes(len(sb.qry(p)), R) >= 2 and len(sb.ref(p)) >= 128]
    assert len(reached) >= 12
    kernel = "k_affine_fill" if algo == "ANW" else "k_linear_fill"
    for wpb in (1, 4):
        env = {"DPX_LANES": "0", "DPX_R": str(R), **({"DPX_WPB": "4"} if wpb == 4 else {})}
        _is(_plan(tool, algo, sb, env), kernel=kernel, rows_per_lane=R, store=0, waves_per_workgroup=wpb, waves=0, couples=0, singles=sb.num_pairs)
    _is(_plan(tool, algo, sb, {"DPX_LANES": "0", "DPX_R": str(R), "DPX_SPLIT": "0", "DPX_PACKED": "0"}, flags=0), kernel=kernel, store=1)


@pytest.mark.parametrize("R", [2, 8])
def test_ties_lie_in_different_stripes(R):
    texts, want = S.tie_want(R)
    assert len(texts) == len(want) == 6


@pytest.mark.parametrize("band", S.BANDS)
def test_the_band_changes_an_answer(tool, oracles, band):
    sb, want = S.band_case(oracles, band)
    assert len(want) == sb.num_pairs
    cpl = 1 if band <= 64 else 2 if band <= 128 else 4 if band <= 256 else 8
    for wpb in (1, 4):
        env = {"DPX_PACKED": "0", **({"DPX_WPB": "4"} if wpb == 4 else {})}
        _is(_plan(tool, "BSW", sb, env, band=band), kernel="k_banded_fill", kernel_algo="BSW", rows_per_lane=cpl, store=0, waves_per_workgroup=wpb, waves=0)


@pytest.mark.parametrize("algo,top", [("LSW", 512), ("LSW", 1024), ("LNW", 1024), ("ANW", 512), ("ASW", 512), ("ASG", 512)])
def test_lane_cases_reach_the_lane_kernels(tool, algo, top):
    sb = S.lane_batch(top)
    affine = algo in ("ANW", "ASW", "ASG")
    kernel = {"ANW": "k_affine_lanes", "ASW": "k_asw_lanes", "ASG": "k_asg_lanes"}.get(algo, "k_linear_lanes")
    f = _plan(tool, algo, sb, {"DPX_LANES": "1"})
    _is(f, kernel=kernel, rows_per_lane=top // 64, store=0, waves_per_workgroup=1 if affine else 4, singles=3, lane_pairs=sb.num_pairs - 3, dtype="int32")
    assert 1 < int(f["waves"]) < sb.num_pairs - 3
    if not affine:
        _is(_plan(tool, algo, sb, {"DPX_LANES": "1", "DPX_WPB": "1"}), kernel=kernel, waves_per_workgroup=1)
    f = _plan(tool, algo, S.ragged40(), {"DPX_LANES": "1"})
    _is(f, kernel=kernel, rows_per_lane=8, store=0, singles=0, lane_pairs=40)
    assert 1 < int(f["waves"]) < 40
