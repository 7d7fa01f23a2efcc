#!/usr/bin/env python3
"""A/B of DPX_ALGO_BAXT (banded affine-gap extension) against DPX_ALGO_BASW and DPX_ALGO_BANW, the two kernels it is put together
from, on the same seeded pairs at the same band: the three alternate (--reps times each, in one process, the order reversed every other
rep; every batch runs one discarded warm-up fill first, then --fills timed fills, dpx_batch_fill_timed).  Workloads: --pairs x 4096^2 at
band 128 and 100 000 short reads (reference 100-160, query 80-130; band 128 admits every pair under BANW), each with matrices and
score-only.  With matrices the fraction of the 8 TB/s HBM roofline from the batch's algorithmic bytes is reported as well.  One JSON
line per measurement, then a summary (median [min, max] of the fill time) that says whether BAXT's median lies inside the [min, max]
of the slower of the other two.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dpx_gpu_genomics_project_amd as dpx  # noqa: E402
from dpx_gpu_genomics_project_amd.synth import make_batch, make_ragged_batch  # noqa: E402

W = (3, -1, -3, -1)
ALGOS = {"BAXT": dpx.ALGO_BAXT, "BASW": dpx.ALGO_BASW, "BANW": dpx.ALGO_BANW}
HBM_BYTES_PER_S = 8e12


def one(name, algo, sb, band, fills, flags):
    with dpx.Batch(ALGOS[algo], sb.sequences, sb.pairs, *W, band=band, flags=flags | dpx.TIME_FILLS) as b:
        b.fill_timed(1)  # warm-up (first touch of the pool, code load): discarded
        us = b.fill_timed(fills)
        info, d = b.info(), b.describe()
        rec = {"workload": name, "algo": algo, "band": band, "kernel": d["kernel"], "cells_per_lane": d["rows_per_lane"], "fill_us": round(us, 1),
               "algorithmic_bytes": info["algorithmic_bytes"], "matrix_bytes": info["matrix_bytes"]}
        if not flags & dpx.SCORE_ONLY:
            rec["roofline_fraction"] = round(info["algorithmic_bytes"] / (us * 1e-6) / HBM_BYTES_PER_S, 3)
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fills", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--band", type=int, default=128)
    ap.add_argument("--short-reads", type=int, default=100000)
    args = ap.parse_args()
    dpx.init(0)
    long_pairs = make_batch(args.pairs, 4096, 4096, seed=43)
    short = make_ragged_batch(args.short_reads, 80, 130, 100, 160, seed=44)
    work = [(f"{args.pairs} x 4096^2", long_pairs, dpx.KEEP_MATRICES), (f"{args.pairs} x 4096^2 score-only", long_pairs, dpx.SCORE_ONLY),
            (f"{args.short_reads} short reads", short, dpx.KEEP_MATRICES), (f"{args.short_reads} short reads score-only", short, dpx.SCORE_ONLY)]
    recs = []
    for name, sb, flags in work:
        for rep in range(args.reps):
            for algo in (list(ALGOS) if rep % 2 == 0 else list(ALGOS)[::-1]):
                recs.append(one(name, algo, sb, args.band, args.fills, flags))
    print(f"summary, band {args.band}: fill time, median [min, max] over {args.reps} batches of {args.fills} fills each")
    for name, _, _ in work:
        stat = {}
        for algo in ALGOS:
            rs = [r for r in recs if r["workload"] == name and r["algo"] == algo]
            v = [r["fill_us"] for r in rs]
            stat[algo] = (statistics.median(v), min(v), max(v))
            roof = f"  roofline {rs[0]['algorithmic_bytes'] / (stat[algo][0] * 1e-6) / HBM_BYTES_PER_S:.3f}" if "roofline_fraction" in rs[0] else ""
            print(f"  {name:36s} {algo:4s} {rs[0]['kernel']:12s} {stat[algo][0] / 1e3:9.3f} ms [{stat[algo][1] / 1e3:.3f}, {stat[algo][2] / 1e3:.3f}]{roof}")
        slower = max(("BASW", "BANW"), key=lambda a: stat[a][0])
        print(f"  {name:36s} BAXT median inside [min, max] of the slower of the two ({slower}): {stat[slower][1] <= stat['BAXT'][0] <= stat[slower][2]}"
              f"; at or below its max: {stat['BAXT'][0] <= stat[slower][2]}")


if __name__ == "__main__":
    main()
