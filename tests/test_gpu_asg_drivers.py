"""The C++ drivers on DPX_ALGO_ASG: dpx_main (batched; -batch / -producer / -directions / -pack2) and dpx_class_main (one AffineSemiGlobal
object per pair from 20 threads, re-ordered with tools/reorder_output.py) on tests/golden/short400.txt print, block for block and byte for
byte, what the CPU oracle tests/asg_oracle.c computes.  Every driver run is a fresh child process with its own timeout."""
import os
import subprocess
import sys

import pytest

import asg_ref
from dpx_gpu_genomics_project_amd.synth import parse_pairs_file

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = os.path.join(ROOT, "tests", "golden", "short400.txt")
HOST = os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "hostcpp")
W = (3, -1, -3, -1)
ARGS = ["-pairs", PAIRS, "-match", "3", "-mismatch", "-1", "-open", "-3", "-extend", "-1", "-algo", "ASG"]


@pytest.fixture(scope="module")
def expected(tmp_path_factory):
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    asg = asg_ref.build(tmp_path_factory.mktemp("asg_drivers"))
    sb = parse_pairs_file(PAIRS)
    assert sb.num_pairs == 400
    return [asg.block(p, sb.ref(p), sb.qry(p), W) for p in range(sb.num_pairs)]


@pytest.mark.parametrize("extra", [[], ["-batch", "37"], ["-batch", "37", "-producer", "2"], ["-directions"], ["-pack2"],
                                   ["-batch", "50", "-directions", "-pack2"]])
def test_dpx_main_asg(expected, extra):
    r = subprocess.run([os.path.join(HOST, "dpx_main")] + ARGS + extra, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout
    body = out[out.index(b"Pair # | Score\n") + len(b"Pair # | Score\n"):out.index(b"Elapsed time (usec): ")]
    assert body == b"".join(expected)


def test_dpx_class_main_asg(expected, tmp_path):
    r = subprocess.run([os.path.join(HOST, "dpx_class_main")] + ARGS, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    raw, ordered = str(tmp_path / "raw.txt"), str(tmp_path / "ordered.txt")
    with open(raw, "wb") as f:
        f.write(r.stdout)
    t = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "reorder_output.py"), raw, ordered], capture_output=True, timeout=60)
    assert t.returncode == 0, t.stderr[-2000:]
    text = open(ordered, "rb").read()
    want = b"".join(expected)
    assert want in text, text[:400]
