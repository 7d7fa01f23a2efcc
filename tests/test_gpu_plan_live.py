"""The library is wired to the planner: a handful of the smallest cases of tests/golden/batch_plans.json as live batches.  For each,
dpx_batch_describe()'s text up to the pool fields and dpx_batch_info() must equal the golden line's, and the filled batch's scores the
oracle's.  The cases run in one process in this order, each with its own knobs in the environment: DPX_SPLIT changes between two
otherwise equal batches, so a knob that stopped arriving would show.  Then one BAXT batch through every setting a batch can change
after its creation, against plan_tool under the matching `mode` line and the zsub oracle."""
import os
import re

import numpy as np
import pytest

import banw_ref
import oracle_py
import plan_cases
import subst_ref
import zsub_ref

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


# One BAXT batch moved through every setting a batch can change after its creation: (setter, arguments, kernel, zdrop, end bonus, table)
SETTINGS = (("plain", None, (), "k_baxt_fill", -1, -1, False),
            ("extension", "set_extension", (2, 3), "k_zext_fill", 2, 3, False),
            ("extension off", "set_extension", (-1, -1), "k_baxt_fill", -1, -1, False),
            ("table", "set_substitution", (), "k_subst_fill", -1, -1, True),
            ("extension + table", "set_extension_table", (2, 3), "k_zsub_fill", 2, 3, True),
            ("end bonus + table", "set_extension_table", (-1, 3), "k_zsub_fill", -1, 3, True))


@pytest.fixture(scope="module")
def zsub(tmp_path_factory):
    return zsub_ref.build(tmp_path_factory.mktemp("plan_live_zsub"))


@pytest.fixture(scope="module")
def tool():
    return plan_cases.build_tool()


@pytest.mark.gpu
@pytest.mark.parametrize("tb_walk", [None, 0], ids=["wave-walk", "lane-walk"])
def test_live_batch_follows_the_route_through_every_setting(gpu, zsub, tool, knobs_of, tb_walk):
    """After each setter the live batch describes itself as plan_tool does for the same case under the matching `mode` line, and its
    fill scores as the zsub oracle does: with an identity table for the settings without one, with Z = E = -1 for extension off
    (tests/test_zsub_oracle.py proves both equivalences).  The last setting's text runs the walk: the wave walk, and under
    DPX_TB_WALK=0 the lane walk."""
    band, gaps, weights = 4, zsub_ref.FUZZ_GAPS, (2, -3)
    texts = [(r, q) for r, q in zsub_ref.fuzz_texts()[band] if 0 < len(r) <= 12 and 0 < len(q) <= 12][:4]
    table, code = np.array(zsub_ref.FUZZ_TABLES[3], np.int8), subst_ref.fuzz_code()
    plain = subst_ref.identity_table(*weights, b"".join(r + q for r, q in texts))
    case = {"name": "route/live", "algo": "BAXT", "weights": [*weights, *gaps], "band": band, "flags": 0,
            "env": {} if tb_walk is None else {"DPX_TB_WALK": tb_walk}, "gen": ["from_strings", [(r.decode(), q.decode()) for r, q in texts]]}
    knobs_of(case)
    sb = plan_cases.make_input(case)
    assert sb.num_pairs == 4
    with gpu.Batch(plan_cases.ALGOS["BAXT"], sb.sequences, sb.pairs, *case["weights"], band=band) as b:
        for tag, setter, args, kernel, Z, E, tabled in SETTINGS:
            if setter:
                getattr(b, setter)(*args, *((table, code) if tabled else ()))
            buf = gpu.capi.C.create_string_buffer(4096)
            assert b._lib.dpx_batch_describe(b._h, buf, 4096) == 0
            text = re.split(r" pool(?:_addr)?=", buf.value.decode())[0]
            want = plan_cases.run_tool(tool, dict(case, mode=[Z, E, table.shape[0] if tabled else 0]))
            assert f" kernel={kernel} " in want and " walk=%s:%d" % ("subst" if tabled else "banw", 2 if tb_walk is None else 0) in want, (tag, want)
            assert "status=0 " + text == want.rsplit(" info=", 1)[0], tag
            b.fill()
            scores = b.results()[0]
            how = (*((table, code) if tabled else plain), *gaps, band, Z, E)
            for p in range(sb.num_pairs):
                assert scores[p] == zsub.align(sb.ref(p), sb.qry(p), *how, walk=False)["score"], (tag, p)
        b.output_begin(0)
        assert b.output_end()[0] == b"".join(zsub.block(p, sb.ref(p), sb.qry(p), table, code, gaps, band, Z, E) for p in range(sb.num_pairs))
