#!/usr/bin/env python3
"""A/B of substitution-matrix scoring (dpx_batch_set_substitution, k_subst_fill) against plain scoring (k_baxt_fill / k_banw_fill,
unchanged code: the yardstick) on ONE batch per workload: the fills alternate between no table and the identity-equivalent table
(scores[a][b] = match if a == b else mismatch over the four base bytes, so both compute the same cells), --reps times each, the order reversed every
other rep, one discarded warm-up fill and then --fills timed fills per measurement (dpx_batch_fill_timed).  Workloads, for BAXT and
BANW: --pairs x 4096^2 at band 128 and a short-extension shape (--short-reads pairs, reference 100-160, query 80-130), each with
matrices and score-only.  Then the walks: on --walk-pairs x 4096^2 the traceback + text kernels (dpx_batch_last_output_usec) of both
walks (DPX_TB_WALK=2 / 0) with and without the table, the batch refilled in front of every measurement.  One JSON line per measurement,
then a summary: median [min, max] and the ratio of the medians.  Needs a GPU."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dpx_gpu_genomics_project_amd as dpx  # noqa: E402
from dpx_gpu_genomics_project_amd.synth import make_batch, make_ragged_batch  # noqa: E402

W = (2, -3, -5, -1)
ALGOS = {"BAXT": dpx.ALGO_BAXT, "BANW": dpx.ALGO_BANW}
MODES = ("plain", "table")


def identity():
    table = np.full((4, 4), W[1], np.int8)
    np.fill_diagonal(table, W[0])
    return table, dpx.code_table(b"0123")  # the synthetic batches write the bases as '0'..'3'


def set_mode(b, mode):
    if mode == "table":
        b.set_substitution(*identity())
    else:
        b.set_substitution(None)


def fills(name, algo, sb, band, reps, nfills, flags):
    recs = []
    with dpx.Batch(ALGOS[algo], sb.sequences, sb.pairs, *W, band=band, flags=flags | dpx.TIME_FILLS) as b:
        for rep in range(reps):
            for mode in (MODES if rep % 2 == 0 else MODES[::-1]):
                set_mode(b, mode)
                b.fill_timed(1)  # warm-up (first touch of the pool, code load): discarded
                us = b.fill_timed(nfills)
                d = b.describe()
                rec = {"workload": name, "algo": algo, "mode": mode, "band": band, "kernel": d["kernel"], "cells_per_lane": d["rows_per_lane"],
                       "fill_us": round(us, 1)}
                print(json.dumps(rec), flush=True)
                recs.append(rec)
    return recs


def walks(name, algo, sb, band, reps, walk):
    os.environ["DPX_TB_WALK"] = str(walk)  # read when the batch is created
    recs = []
    lib = dpx.load()
    with dpx.Batch(ALGOS[algo], sb.sequences, sb.pairs, *W, band=band, flags=dpx.KEEP_MATRICES | dpx.TIME_FILLS) as b:
        for rep in range(reps + 1):  # the first round of both modes is the warm-up
            for mode in (MODES if rep % 2 == 0 else MODES[::-1]):
                set_mode(b, mode)
                b.fill()
                b.output_begin(0)
                b.output_end()
                us = C.c_double()
                assert lib.dpx_batch_last_output_usec(b._h, C.byref(us)) == 0
                if rep:
                    rec = {"workload": name, "algo": algo, "mode": mode, "band": band, "kernel": b.describe()["traceback"], "fill_us": round(us.value, 1)}
                    print(json.dumps(rec), flush=True)
                    recs.append(rec)
    del os.environ["DPX_TB_WALK"]
    return recs


def summary(recs):
    for key in dict.fromkeys((r["workload"], r["algo"]) for r in recs):
        stat, kern = {}, {}
        for mode in MODES:
            v = [r["fill_us"] for r in recs if (r["workload"], r["algo"]) == key and r["mode"] == mode]
            stat[mode] = (statistics.median(v), min(v), max(v))
            kern[mode] = next(r["kernel"] for r in recs if (r["workload"], r["algo"]) == key and r["mode"] == mode)
            print(f"  {key[0]:40s} {key[1]:4s} {kern[mode]:24s} {stat[mode][0] / 1e3:9.3f} ms [{stat[mode][1] / 1e3:.3f}, {stat[mode][2] / 1e3:.3f}]")
        print(f"  {key[0]:40s} {key[1]:4s} table median / plain median: {stat['table'][0] / stat['plain'][0]:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fills", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--band", type=int, default=128)
    ap.add_argument("--short-reads", type=int, default=100000)
    ap.add_argument("--walk-pairs", type=int, default=1712)
    args = ap.parse_args()
    dpx.init(0)
    long_pairs = make_batch(args.pairs, 4096, 4096, seed=43)
    short = make_ragged_batch(args.short_reads, 80, 130, 100, 160, seed=44)
    recs = []
    for algo in ALGOS:
        for name, sb in ((f"{args.pairs} x 4096^2", long_pairs), (f"{args.short_reads} short extensions", short)):
            recs += fills(name, algo, sb, args.band, args.reps, args.fills, dpx.KEEP_MATRICES)
            recs += fills(name + " score-only", algo, sb, args.band, args.reps, args.fills, dpx.SCORE_ONLY)
    walk_pairs = make_batch(args.walk_pairs, 4096, 4096, seed=46)
    for algo in ALGOS:
        for walk, label in ((2, "wave walk"), (0, "lane walk")):
            recs += walks(f"{args.walk_pairs} x 4096^2 {label} + text", algo, walk_pairs, args.band, args.reps, walk)
    print(f"summary, band {args.band}: median [min, max] over {args.reps} measurements ({args.fills} fills each; walks: one traceback + text each)")
    summary(recs)


if __name__ == "__main__":
    main()
