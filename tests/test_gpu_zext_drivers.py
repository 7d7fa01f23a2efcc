"""dpx_main on BAXT's extension mode: with -zdrop 20 -endbonus 5 at band 33 it prints, block for block and byte for byte, what the CPU
oracle tests/zext_oracle.c computes on a small ragged batch written by the test (shared starts with 8 % substitutions and unrelated
tails, so most pairs drop, and a few near-end-mismatch pairs that the bonus carries to the end of the query); with another algorithm
the two flags end in the usage text."""
import os
import subprocess

import numpy as np
import pytest

import zext_ref
from dpx_gpu_genomics_project_amd.synth import from_strings, parse_pairs_file, write_pairs_file

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "hostcpp")
W = (2, -3, -5, -1)
BAND, Z, E = 33, 20, 5
COUNT = 60


def _pairs():
    rng = np.random.default_rng(78)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    texts = []
    for k in range(COUNT):
        if k % 10 == 9:  # the reference's first 60 bases with substitutions at m-2, m-4, m-6
            ref = rng.integers(0, 4, 80)
            q = ref[:60].copy()
            for at in (58, 56, 54):
                q[at] = (q[at] + 1) % 4
        else:
            pre = rng.integers(0, 4, int(rng.integers(0, 121)))
            q = pre.copy()
            sub = rng.random(len(q)) < 0.08
            q[sub] = rng.integers(0, 4, int(sub.sum()))
            ref = np.concatenate([pre, rng.integers(0, 4, int(rng.integers(1, 90)))])
            q = np.concatenate([q, rng.integers(0, 4, int(rng.integers(1, 60)))])
        texts.append((acgt[ref].tobytes(), acgt[q].tobytes()))
    return from_strings(texts)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    tmp = tmp_path_factory.mktemp("zext_drivers")
    path = str(tmp / "pairs.txt")
    write_pairs_file(_pairs(), path)
    sb = parse_pairs_file(path)
    assert sb.num_pairs == COUNT
    zext = zext_ref.build(tmp)
    flags = [zext.align(sb.ref(p), sb.qry(p), *W, BAND, Z, E, walk=False)["rec"]["flags"] for p in range(COUNT)]
    assert sum(f == zext_ref.ZDROPPED for f in flags) >= COUNT // 3 and sum(f == zext_ref.REACHED_END for f in flags) >= COUNT // 10, flags
    args = ["-pairs", path, "-match", str(W[0]), "-mismatch", str(W[1]), "-open", str(W[2]), "-extend", str(W[3]), "-band", str(BAND)]
    return args, [zext.block(p, sb.ref(p), sb.qry(p), W, BAND, Z, E) for p in range(COUNT)]


@pytest.mark.parametrize("extra", [[], ["-pack2"], ["-batch", "7"]])
def test_dpx_main_zext(case, extra):
    args, expected = case
    r = subprocess.run([os.path.join(HOST, "dpx_main")] + args + ["-algo", "BAXT", "-zdrop", str(Z), "-endbonus", str(E)] + extra,
                       capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = r.stdout
    body = out[out.index(b"Pair # | Score\n") + len(b"Pair # | Score\n"):out.index(b"Elapsed time (usec): ")]
    assert body == b"".join(expected)


def test_dpx_main_refuses_the_flags_elsewhere(case):
    args, _ = case
    r = subprocess.run([os.path.join(HOST, "dpx_main")] + args + ["-algo", "BASW", "-zdrop", str(Z), "-endbonus", str(E)], capture_output=True, timeout=600)
    assert r.returncode != 0 and r.stderr.startswith(b"usage: dpx_main") and b"-zdrop" in r.stderr and b"Pair #" not in r.stdout
