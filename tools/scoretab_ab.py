#!/usr/bin/env python3
"""A/B of ANW / ASW / ASG score-only batches under dpx_batch_set_score_table (k_scoretab_fill / k_scoretab_lanes) after
tools/dirtab_ab.py's method.  Per workload, in one process:
  (a) ONE score-only batch, filled plain and under the identity-equivalent table (match on the diagonal, mismatch elsewhere, an injective
      byte map, so both fills compute the same cells and the child checks that the results agree), the two alternating: set the table,
      then clear it (--reps times each, the order reversed every other rep; one discarded warm-up fill, then --fills timed fills per
      measurement, dpx_batch_fill_timed);
  (b) the same pairs and table on a DPX_KEEP_DIRECTIONS batch (k_dirtab_fill, dpx_batch_set_direction_table): what a caller who wanted
      scores under a table had to run before.  The feature's claim is (a)'s table fill against this one.
Workloads: --pairs x 1024^2 for each of ANW, ASW and ASG over ACGT; --protein-pairs pairs of 350 x 350 over 24 letters (ASW);
--short-reads short reads (reference 100-160, query 80-130; the lane-packed kernels), ASW and ASG; one 350-residue query against
--search-refs references of 50-1000 residues over 24 letters (ASW; every pair's query is the same byte range).

The parent process starts --processes fresh child processes one after the other, each under its own timeout (it never opens the GPU
itself, and a child that fails or hangs ends the run), and prints per workload and mode the median [min, max] of the children's
medians and the ratios of the medians.  --package-root DIR measures with the package of another checkout (the parent commit's, say):
where its library has no dpx_batch_set_score_table only the plain score-only fill is timed, which is how (c), the plain kernels of two
commits, is compared on one machine.  Needs a GPU.  A measurement tool: it is not run as a test and gates nothing."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = (3, -1, -3, -1)
MODES = ("plain", "table", "dirtab")
PROTEIN = b"ARNDCQEGHILKMFPSTWYVBZX*"


def identity(letters):
    """(scores, code_of) that score exactly as byte equality does over `letters`"""
    code = np.zeros(256, np.uint8)
    for k, ch in enumerate(sorted(set(letters))):
        code[ch] = k
    table = np.full((len(set(letters)),) * 2, W[1], np.int8)
    np.fill_diagonal(table, W[0])
    return table, code


def related(count, n, m, letters, seed):
    """`count` pairs: the query copies the reference with 10 % substitutions"""
    from dpx_gpu_genomics_project_amd.synth import from_strings

    rng = np.random.default_rng(seed)
    abc = np.frombuffer(letters, np.uint8)
    texts = []
    for _ in range(count):
        ref = rng.integers(0, len(abc), n)
        q = np.resize(ref, m).copy()
        sub = rng.random(m) < 0.10
        q[sub] = rng.integers(0, len(abc), int(sub.sum()))
        texts.append((abc[ref].tobytes(), abc[q].tobytes()))
    return from_strings(texts)


class Search:
    """one query of `m` residues against `count` references of 50-1000: every pair's query is the same byte range"""

    def __init__(self, count, m, letters, seed):
        from dpx_gpu_genomics_project_amd.capi import PAIR_DTYPE

        rng = np.random.default_rng(seed)
        abc = np.frombuffer(letters, np.uint8)
        lens = rng.integers(50, 1001, count)
        starts = m + np.concatenate([[0], np.cumsum(lens)[:-1]])
        self.sequences = abc[rng.integers(0, len(abc), m + int(lens.sum()))]
        self.pairs = np.zeros(count, PAIR_DTYPE)
        self.pairs["referenceIdx"], self.pairs["referenceSize"], self.pairs["queryIdx"], self.pairs["querySize"] = starts, lens, 0, m


def child(args):
    sys.path.insert(0, os.path.abspath(args.package_root) if args.package_root else ROOT)
    import dpx_gpu_genomics_project_amd as dpx
    from dpx_gpu_genomics_project_amd.synth import make_ragged_batch

    dpx.init(0)
    has_table = hasattr(dpx.Batch, "set_score_table") and hasattr(dpx.load(), "dpx_batch_set_score_table")
    algos = {"ANW": dpx.ALGO_ANW, "ASW": dpx.ALGO_ASW, "ASG": dpx.ALGO_ASG}
    square = related(args.pairs, 1024, 1024, b"ACGT", 43)
    work = [(f"{args.pairs} x 1024^2", algo, square, b"ACGT") for algo in algos]
    work.append((f"{args.protein_pairs} x 350^2, 24 letters", "ASW", related(args.protein_pairs, 350, 350, PROTEIN, 45), PROTEIN))
    reads = make_ragged_batch(args.short_reads, 80, 130, 100, 160, seed=44)
    work += [(f"{args.short_reads} short reads", algo, reads, b"0123") for algo in ("ASW", "ASG")]
    work.append((f"350 against {args.search_refs} references of 50-1000", "ASW", Search(args.search_refs, 350, PROTEIN, 46), PROTEIN))
    for name, algo, sb, letters in work:
        table, code = identity(letters)
        results = {}

        def measure(b, mode):
            b.fill_timed(1)  # warm-up (code load, first touch of a pool): discarded
            us = b.fill_timed(args.fills)
            d = b.describe()
            if mode not in results:
                results[mode] = [x.copy() for x in b.results()]
            rec = {"workload": name, "algo": algo, "mode": mode, "kernel": d["kernel"], "rows_per_lane": d["rows_per_lane"], "subst": d.get("subst", 0),
                   "waves_per_workgroup": d["waves_per_workgroup"], "fill_us": round(us, 1), "pool_bytes": b.info()["matrix_bytes"]}
            print(json.dumps(rec), flush=True)

        with dpx.Batch(algos[algo], sb.sequences, sb.pairs, *W, flags=dpx.SCORE_ONLY) as b:
            modes = MODES[:2] if has_table else MODES[:1]
            for rep in range(args.reps):
                for mode in (modes if rep % 2 == 0 else modes[::-1]):
                    if has_table:
                        b.set_score_table(*((table, code) if mode == "table" else (None,)))
                    measure(b, mode)
        if has_table and not args.no_directions:
            with dpx.Batch(algos[algo], sb.sequences, sb.pairs, *W, flags=dpx.KEEP_DIRECTIONS) as b:
                b.set_direction_table(table, code)
                for rep in range(args.reps):
                    measure(b, "dirtab")
        for mode in results:  # the identity-equivalent table: the same scores and end cells everywhere
            assert all(np.array_equal(x, y) for x, y in zip(results["plain"], results[mode])), (name, mode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--fills", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--short-reads", type=int, default=100000)
    ap.add_argument("--protein-pairs", type=int, default=10000)
    ap.add_argument("--search-refs", type=int, default=100000)
    ap.add_argument("--no-directions", action="store_true", help="skip (b), the direction batch")
    ap.add_argument("--package-root", default=None, help="measure with the package of this checkout instead (plain fill only where it has no table)")
    ap.add_argument("--child-timeout", type=float, default=300.0, help="seconds after which a child process is killed")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    recs = []
    for proc in range(args.processes):
        # (every GPU step under its own time limit; a failed or hung child raises here and ends the run: nothing more is started on the card)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"],
                             capture_output=True, text=True, check=True, timeout=args.child_timeout).stdout
        for line in out.splitlines():
            rec = json.loads(line)
            rec["process"] = proc
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    where = f" with the package of {args.package_root}" if args.package_root else ""
    print(f"summary{where}: fill time, median [min, max] over {args.processes} fresh processes of each process's median "
          f"({args.reps} measurements of {args.fills} fills), weights {W}")
    for key in dict.fromkeys((r["workload"], r["algo"]) for r in recs):
        med = {}
        for mode in MODES:
            mine = [r for r in recs if (r["workload"], r["algo"]) == key and r["mode"] == mode]
            if not mine:
                continue
            per = [statistics.median([r["fill_us"] for r in mine if r["process"] == p]) for p in range(args.processes)]
            med[mode], first = statistics.median(per), mine[0]
            ratio = f"  x{med[mode] / med['plain']:.3f} of plain" if mode == "table" else ""
            ratio = f"  score-only table fill x{med['table'] / med[mode]:.3f} of this" if mode == "dirtab" and "table" in med else ratio
            print(f"  {key[0]:44s} {key[1]:3s} {mode:6s} {first['kernel']:14s} R {first['rows_per_lane']} subst {first['subst']:2d} wpb {first['waves_per_workgroup']} "
                  f"{med[mode] / 1e3:9.3f} ms [{min(per) / 1e3:.3f}, {max(per) / 1e3:.3f}]  pool {first['pool_bytes']}{ratio}")


if __name__ == "__main__":
    main()
