#!/usr/bin/env python3
"""A/B of BAXT's extension mode (dpx_batch_set_extension, k_zext_fill) against plain DPX_ALGO_BAXT (k_baxt_fill) on the same seeded
pairs at the same band: the two alternate (--reps times each, in one process, the order reversed every other rep; every batch runs one
discarded warm-up fill first, then --fills timed fills, dpx_batch_fill_timed).  Workloads: --pairs x 4096^2 at band 128, once fully
related (8 % substitutions; with --zdrop 400 nothing drops, so the difference is the cost of the per-step test) and once related for the
first 1024 bases only (the pairs drop; the mean lastDiag of the batch is printed beside the time), and 100 000 short reads (reference
100-160, query 80-130), each with matrices and score-only.  The extension mode runs as (Z, -1): the kernel with the drop test.  One JSON
line per measurement, then a summary (median [min, max] of the fill time) that says whether the extension mode's median on the
never-dropping batch is no worse than BAXT's median plus BAXT's own min-to-max spread.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dpx_gpu_genomics_project_amd as dpx  # noqa: E402
from dpx_gpu_genomics_project_amd.synth import from_strings, make_ragged_batch  # noqa: E402

W = (2, -3, -5, -1)
MODES = ("BAXT", "ZEXT")


def related(count, size, shared, seed):
    """`count` pairs of `size` bases: the query copies the reference's first `shared` bases with 8 % substitutions, the rest is random"""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    texts = []
    for _ in range(count):
        ref = rng.integers(0, 4, size)
        q = rng.integers(0, 4, size)
        q[:shared] = ref[:shared]
        sub = rng.random(shared) < 0.08
        q[:shared][sub] = rng.integers(0, 4, int(sub.sum()))
        texts.append((acgt[ref].tobytes(), acgt[q].tobytes()))
    return from_strings(texts)


def one(name, mode, sb, band, zdrop, fills, flags):
    with dpx.Batch(dpx.ALGO_BAXT, sb.sequences, sb.pairs, *W, band=band, flags=flags | dpx.TIME_FILLS) as b:
        if mode == "ZEXT":
            b.set_extension(zdrop, -1)
        b.fill_timed(1)  # warm-up (first touch of the pool, code load): discarded
        us = b.fill_timed(fills)
        d = b.describe()
        rec = {"workload": name, "mode": mode, "band": band, "kernel": d["kernel"], "cells_per_lane": d["rows_per_lane"], "fill_us": round(us, 1)}
        if mode == "ZEXT":
            ext = b.extensions()
            rec["zdrop"] = zdrop
            rec["dropped"] = int(np.sum((ext["flags"] & dpx.EXT_ZDROPPED) != 0))
            rec["mean_last_diag"] = round(float(np.mean(ext["lastDiag"])), 1)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fills", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--band", type=int, default=128)
    ap.add_argument("--zdrop", type=int, default=400)
    ap.add_argument("--short-reads", type=int, default=100000)
    args = ap.parse_args()
    dpx.init(0)
    full = related(args.pairs, 4096, 4096, seed=43)
    part = related(args.pairs, 4096, 1024, seed=45)
    short = make_ragged_batch(args.short_reads, 80, 130, 100, 160, seed=44)
    work = []
    for name, sb in ((f"{args.pairs} x 4096^2 related", full), (f"{args.pairs} x 4096^2 related for 1024", part), (f"{args.short_reads} short reads", short)):
        work += [(name, sb, dpx.KEEP_MATRICES), (name + " score-only", sb, dpx.SCORE_ONLY)]
    recs = []
    for name, sb, flags in work:
        for rep in range(args.reps):
            for mode in (MODES if rep % 2 == 0 else MODES[::-1]):
                recs.append(one(name, mode, sb, args.band, args.zdrop, args.fills, flags))
    print(f"summary, band {args.band}, Z = {args.zdrop}: fill time, median [min, max] over {args.reps} batches of {args.fills} fills each")
    for name, _, _ in work:
        stat = {}
        for mode in MODES:
            rs = [r for r in recs if r["workload"] == name and r["mode"] == mode]
            v = [r["fill_us"] for r in rs]
            stat[mode] = (statistics.median(v), min(v), max(v))
            tail = f"  dropped {rs[0]['dropped']}, mean lastDiag {rs[0]['mean_last_diag']}" if mode == "ZEXT" else ""
            print(f"  {name:44s} {rs[0]['kernel']:12s} {stat[mode][0] / 1e3:9.3f} ms [{stat[mode][1] / 1e3:.3f}, {stat[mode][2] / 1e3:.3f}]{tail}")
        bound = stat["BAXT"][0] + (stat["BAXT"][2] - stat["BAXT"][1])
        print(f"  {name:44s} k_zext_fill median / k_baxt_fill median: {stat['ZEXT'][0] / stat['BAXT'][0]:.3f}; "
              f"at or below BAXT's median plus its spread: {stat['ZEXT'][0] <= bound}")


if __name__ == "__main__":
    main()
