"""The batch planner (csrc/dpx_plan.cpp) on the CPU: hostcpp/plan_tool runs every case of tests/golden/batch_plans.json and must print
the line that the commit before the planner existed produced for the same input on a real device (profiles/plan_split.md): status, error
text, dpx_batch_describe()'s text up to the pool fields, dpx_batch_info()'s numbers and a hash of everything the kernels are told."""
import pytest

import plan_cases

CASES = plan_cases.load_cases()
KERNELS = {"k_linear_fill", "k_linear_fill_pk", "k_linear_lanes", "k_linear_lanes_pk", "k_linear_split", "k_affine_fill", "k_asw_fill",
           "k_asg_fill", "k_affine_lanes", "k_asw_lanes", "k_asg_lanes", "k_banded_fill", "k_banded_fill_pk", "k_basw_fill", "k_banw_fill",
           "k_baxt_fill", "k_bdir_fill", "k_linear_dir", "k_affine_dir", "k_asw_dir", "k_asg_dir"}


@pytest.fixture(scope="module")
def tool():
    return plan_cases.build_tool()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_plan_matches_the_recorded_batch(tool, case):
    assert case["expect"].startswith("status="), "the golden line was never recorded"
    assert plan_cases.run_tool(tool, case) == case["expect"]


def test_golden_covers_every_create_time_kernel():
    seen = {kv.split("=", 1)[1] for c in CASES for kv in c["expect"].split() if kv.startswith("kernel=")}
    assert seen == KERNELS


def test_golden_holds_every_refusal_kind():
    statuses = {c["expect"].split()[0] for c in CASES}
    assert {"status=0", "status=-1", "status=-4", "status=-8"} <= statuses  # ok, invalid, range, unsupported
    assert any("needs band >= 11, the batch has band 10" in c["expect"] for c in CASES)
