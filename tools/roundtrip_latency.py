#!/usr/bin/env python3
"""roundtrip_latency.py -- host cost of one whole small-batch round trip, in microseconds: dpx_batch_create, dpx_batch_fill,
dpx_batch_output_begin / _end, dpx_batch_results and dpx_batch_destroy of a 20-pair LNW batch with matrices (reads of about 100 x 120),
as the class-per-pair drivers make them by the thousand.  Every buffer comes out of the library's caches after the first trip, so this is
the path a change to the host side of the library (csrc/dpx_capi.cpp, dpx_output.cpp, dpx_mem.cpp) can slow down.

DPX_LIB chooses the library (tools/ A-B runs: alternate fresh processes of two builds on one machine).  --trips round trips (default
500) after --warmup (default 100); prints one JSON line: the median, the quartiles and the minimum."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dpx_gpu_genomics_project_amd as dpx  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--trips", type=int, default=500)
ap.add_argument("--warmup", type=int, default=100)
args = ap.parse_args()

dpx.init(0)
sb = dpx.make_batch(20, 100, 120, seed=6)


def trip():
    with dpx.Batch(dpx.ALGO_LNW, sb.sequences, sb.pairs, 3, -1, -2) as b:
        b.fill()
        b.output_begin(0)
        text, _ = b.output_end()
        scores, _, _ = b.results()
        return len(text), int(scores[0])


first = trip()
for _ in range(args.warmup):
    trip()
times = []
for _ in range(args.trips):
    t0 = time.perf_counter()
    got = trip()
    times.append((time.perf_counter() - t0) * 1e6)
    assert got == first
q = statistics.quantiles(times, n=4)
print(json.dumps({"lib": os.environ.get("DPX_LIB", ""), "trips": args.trips, "median_us": round(statistics.median(times), 2),
                  "q1_us": round(q[0], 2), "q3_us": round(q[2], 2), "min_us": round(min(times), 2)}))
