"""The batch-plan cases of tests/golden/batch_plans.json: how a case becomes a pair table, plan_tool's input and a live batch.

A case is a dict: name; algo (name), weights [match, mismatch, gapOpen, gapExtend], band, flags; env (the DPX_* knobs set for it); gen, a
call of synth.make_batch / make_ragged_batch / from_strings as [function name, arguments...]; optionally tweak, a list of
[pair, field, value] applied to the generated pair table (an empty or an invalid pair inside a regular batch), first_pair, packed2
(the sequences go in as 2-bit codes), and mode, [zdrop, endBonus, substAlphabet] as the setters of a live batch would leave them
(plan_tool then prints the walk as well; no golden case has one).  expect is the line plan_tool must print, recorded from the commit before the planner existed
(profiles/plan_split.md)."""
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "batch_plans.json")
HOSTCPP = os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "hostcpp")
# plan_tool's `knobs` line, in order, with the value refresh_knobs() gives an unset variable
KNOBS = (("DPX_R", 0), ("DPX_PACKED", -1), ("DPX_LANES", -1), ("DPX_LANES_PK", -1), ("DPX_SPLIT", -1), ("DPX_ROW_TAGS", -1),
         ("DPX_RAMP_LINES", -1), ("DPX_WPB", 0), ("DPX_GROUP", 0), ("DPX_TB_WALK", -1))
ALGOS = {"LNW": 0, "LSW": 1, "ANW": 2, "BSW": 3, "ASW": 4, "BASW": 5, "ASG": 6, "BANW": 7, "BAXT": 10}


def load_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def write_cases(path, cases):
    """One case per line, so that a diff of the golden file reads case by case."""
    with open(path, "w") as f:
        f.write('{"cases": [\n' + ",\n".join(json.dumps(c) for c in cases) + "\n]}\n")


def make_input(case):
    """The SynthBatch of a case (tweaks applied to its pair table)."""
    from dpx_gpu_genomics_project_amd import synth

    name, *args = case["gen"]
    assert name in ("make_batch", "make_ragged_batch", "from_strings"), name
    sb = getattr(synth, name)(*([[tuple(p) for p in args[0]]] if name == "from_strings" else args))
    for pair, field, value in case.get("tweak", []):
        sb.pairs[pair][field] = value
    return sb


def tool_input(case, sb) -> str:
    env = case.get("env", {})
    assert set(env) <= {k for k, _ in KNOBS}, env
    first = case.get("first_pair", 0)
    head = ["params %d %d %d %d %d %d" % (ALGOS[case["algo"]], *case["weights"], case["band"]), "flags %d" % case["flags"],
            "knobs " + " ".join(str(int(env.get(k, unset))) for k, unset in KNOBS),
            "input %d %d %d %d" % (1 if case.get("packed2") else 0, sb.sequences.size, first, len(sb.pairs) - first)]
    if "mode" in case:
        head.append("mode %d %d %d" % tuple(case["mode"]))
    p = sb.pairs
    table = np.stack([p["referenceIdx"], p["referenceSize"], p["queryIdx"], p["querySize"]], axis=1).astype(np.int64)
    return "\n".join(head) + "\n" + "\n".join(" ".join(map(str, row)) for row in table.tolist()) + "\n"


def build_tool(make_args=(), exe="plan_tool") -> str:
    subprocess.run(["make", "-s", "-C", HOSTCPP, "plan_tool", *make_args], check=True)
    return os.path.join(HOSTCPP, exe)


def run_tool(exe: str, case) -> str:
    r = subprocess.run([exe], input=tool_input(case, make_input(case)), capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (case["name"], r.returncode, r.stderr[-2000:])
    return r.stdout.rstrip("\n")
