"""The library is wired to the planner: a handful of the smallest cases of tests/golden/batch_plans.json as live batches.  For each,
dpx_batch_describe()'s text up to the pool fields and dpx_batch_info() must equal the golden line's, and the filled batch's scores the
oracle's.  The cases run in one process in this order, each with its own knobs in the environment: DPX_SPLIT changes between two
otherwise equal batches, so a knob that stopped arriving would show."""
import os
import re

import pytest

import banw_ref
import oracle_py
import plan_cases

LIVE = ("rows/linear/m128", "lanes/DPX_LANES1", "packed/DPX_PACKED1", "split/default", "split/DPX_SPLIT0", "rows/dir/m128",
        "banddir/small", "plain/score_only")
CASES = {c["name"]: c for c in plan_cases.load_cases()}
KERNEL = {"rows/linear/m128": "k_linear_fill", "lanes/DPX_LANES1": "k_linear_lanes_pk", "packed/DPX_PACKED1": "k_linear_fill_pk",
          "split/default": "k_linear_split", "split/DPX_SPLIT0": "k_linear_fill", "rows/dir/m128": "k_linear_dir",
          "banddir/small": "k_bdir_fill", "plain/score_only": "k_linear_fill"}


@pytest.fixture(scope="module")
def banw(tmp_path_factory):
    return banw_ref.build(tmp_path_factory.mktemp("plan_live_banw"))


@pytest.fixture
def knobs_of():
    saved = {k: os.environ.get(k) for k, _ in plan_cases.KNOBS}

    def apply(case):
        for k, _ in plan_cases.KNOBS:
            os.environ.pop(k, None)
        os.environ.update({k: str(v) for k, v in case["env"].items()})

    yield apply
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


@pytest.mark.gpu
@pytest.mark.parametrize("name", LIVE)
def test_live_batch_follows_the_plan(gpu, banw, knobs_of, name):
    case = CASES[name]
    golden = case["expect"]
    assert f" kernel={KERNEL[name]} " in golden
    knobs_of(case)
    sb = plan_cases.make_input(case)
    w = case["weights"]
    with gpu.Batch(plan_cases.ALGOS[case["algo"]], sb.sequences, sb.pairs, *w, band=case["band"], flags=case["flags"]) as b:
        buf = gpu.capi.C.create_string_buffer(4096)
        assert b._lib.dpx_batch_describe(b._h, buf, 4096) == 0
        text = re.split(r" pool(?:_addr)?=", buf.value.decode())[0]
        info = b.info()
        line = "status=0 %s info=%d,%d,%d,%d" % (text, info["num_pairs"], info["cells"], info["matrix_bytes"], info["algorithmic_bytes"])
        assert line == golden.rsplit(" state=", 1)[0]
        b.fill()
        scores = b.results()[0]
    for p in range(sb.num_pairs):
        if case["algo"] == "BANW":
            want = banw.align(sb.ref(p), sb.qry(p), *w, case["band"])["score"]
        else:
            want = oracle_py.lsw(sb.ref(p), sb.qry(p), w[0], w[1], w[2], want_dir=False).score
        assert scores[p] == want, (name, p)
