"""dpx_main -scores: score-only batches from the driver.  -algo ANW|ASW|ASG -scores -matrix FILE goes through dpx_batch_set_score_table
and prints, line for line, "<number> | <score> | <endRow> <endCol>" as the CPU oracle tests/dirtab_oracle.c computes them under the
file's table; -scores without -matrix prints what the plain score-only batch's results give (LSW and ANW); the documented usage errors
exit non-zero with nothing on stdout.  Every driver run is a fresh child process with its own timeout."""
import os
import subprocess

import numpy as np
import pytest

import dirtab_ref
from dpx_gpu_genomics_project_amd.synth import from_strings, write_pairs_file

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "hostcpp")
GAPS = (-5, -1)
COUNT = 60
LETTERS = "ACGTN"
# rows: the reference's letter.  Asymmetric (transitions cost less one way round), and N against anything, N included, is negative
TABLE = np.array([[4, -6, -2, -6, -1], [-6, 4, -6, -3, -1], [-1, -6, 4, -6, -1], [-6, -2, -6, 4, -1], [-1, -1, -1, -1, -1]], np.int8)


def _code():
    """dpx_main's map for the file: a letter and its lower case take the letter's code, every other byte the last letter's"""
    code = np.full(256, len(LETTERS) - 1, np.uint8)
    for k, ch in enumerate(LETTERS):
        code[ord(ch)] = code[ord(ch.lower())] = k
    return code


def _pairs():
    rng = np.random.default_rng(98)
    letters = np.frombuffer(b"ACGTACGTACGTN", np.uint8)
    texts = []
    for k in range(COUNT):
        n, m = int(rng.integers(1, 150)), int(rng.integers(1, 150))
        ref = rng.integers(0, len(letters), n)
        q = np.resize(ref[int(rng.integers(0, max(n // 3, 1))):], m).copy()
        hit = rng.random(m) < 0.12
        q[hit] = rng.integers(0, len(letters), int(hit.sum()))
        texts.append((letters[ref].tobytes(), letters[q].tobytes()))
    return from_strings(texts)


def _lines(results):
    return b"".join(b"%d | %d | %d %d\n" % (p, s, r, c) for p, (s, r, c) in enumerate(results))


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    subprocess.run(["make", "-s", "-C", HOST], check=True)
    tmp = tmp_path_factory.mktemp("scoretab_drivers")
    dt = dirtab_ref.build(tmp)
    sb = _pairs()
    pairs = str(tmp / "pairs.txt")
    write_pairs_file(sb, pairs)
    matrix = str(tmp / "acgtn.txt")
    with open(matrix, "w") as f:
        f.write("# rows: the reference's letter\n  " + " ".join(LETTERS) + "\n")
        for k, letter in enumerate(LETTERS):
            f.write(letter + " " + " ".join(str(int(v)) for v in TABLE[k]) + "\n")
    want = {}
    for kind in ("ANW", "ASW", "ASG"):
        res = [dt.align(kind, sb.ref(p), sb.qry(p), TABLE, _code(), *GAPS) for p in range(sb.num_pairs)]
        want[kind] = _lines([(r["score"], *r["end"]) for r in res])
    assert want["ANW"] != want["ASG"] != want["ASW"]
    return pairs, matrix, want, sb


def _run(pairs, extra):
    args = ["-pairs", pairs, "-match", "2", "-mismatch", "-3", "-open", str(GAPS[0]), "-extend", str(GAPS[1])]
    r = subprocess.run([os.path.join(HOST, "dpx_main")] + args + extra, capture_output=True, timeout=300)
    assert r.returncode == 0, (extra, r.stderr[-2000:])
    out = r.stdout
    return out[out.index(b"Pair # | Score\n") + len(b"Pair # | Score\n"):out.index(b"Elapsed time (usec): ")]


@pytest.mark.parametrize("kind", ["ANW", "ASW", "ASG"])
def test_dpx_main_prints_the_oracle_lines(case, kind):
    pairs, matrix, want, _ = case
    base = ["-algo", kind, "-scores", "-matrix", matrix]
    assert _run(pairs, base) == want[kind]
    assert _run(pairs, base + ["-batch", "17"]) == want[kind]


@pytest.mark.parametrize("algo", ["LSW", "ANW"])
def test_scores_without_a_matrix_prints_the_plain_results(gpu, case, algo):
    pairs, _, _, sb = case
    with gpu.Batch({"LSW": gpu.ALGO_LSW, "ANW": gpu.ALGO_ANW}[algo], sb.sequences, sb.pairs, 2, -3, *GAPS, flags=gpu.SCORE_ONLY) as b:
        b.fill()
        s, r, c = b.results()
    assert _run(pairs, ["-algo", algo, "-scores"]) == _lines(zip(s.tolist(), r.tolist(), c.tolist()))


def test_usage_errors_print_nothing(case):
    pairs, matrix, _, _ = case
    for extra in (["-algo", "ASW", "-scores", "-directions"], ["-algo", "ASW", "-scores", "-cigar"], ["-algo", "BAXT", "-scores", "-zdrop", "10"],
                  ["-algo", "BAXT", "-scores", "-endbonus", "3"], ["-algo", "BANW", "-scores", "-reverse"],
                  ["-algo", "BANW", "-scores", "-open2", "-3", "-extend2", "-1"], ["-algo", "LSW", "-scores", "-matrix", matrix],
                  ["-algo", "BANW", "-scores", "-matrix", matrix], ["-algo", "BASW", "-scores", "-matrix", matrix]):
        r = subprocess.run([os.path.join(HOST, "dpx_main"), "-pairs", pairs, "-open", "-5", "-extend", "-1"] + extra, capture_output=True, timeout=120)
        assert r.returncode != 0 and r.stderr.startswith(b"usage: dpx_main") and r.stdout == b"", extra
