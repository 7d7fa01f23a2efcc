#!/usr/bin/env python3
"""fill_latency.py -- host cost of dpx_batch_fill() on a tiny batch (the class-per-pair drivers fill thousands of them), in microseconds.

DPX_LIB chooses the library (tools/ A-B runs).  One LNW pair of 100 x 120, 500 warm-up fills, then
  enqueue_us: 20 000 fills back to back, host time per call before the final dpx_batch_sync (median of 5 rounds; with the queue this long the
              figure may be the rate at which the device takes them)
  burst_us: 16 fills into an empty queue, host time per call (median of 1000 bursts): the host side of a call alone
  fill_sync_us: one fill and one dpx_batch_sync, median of 2000
Prints one JSON line."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dpx_gpu_genomics_project_amd as dpx  # noqa: E402

dpx.init(0)
sb = dpx.make_batch(1, 100, 120, seed=6)
with dpx.Batch(dpx.ALGO_LNW, sb.sequences, sb.pairs, 3, -1, -2) as b:
    fill, h = b._lib.dpx_batch_fill, b._h
    for _ in range(500):
        fill(h, None)
    b.sync()
    rounds = []
    for _ in range(5):
        t0 = time.perf_counter()
        for _ in range(20000):
            fill(h, None)
        rounds.append((time.perf_counter() - t0) / 20000 * 1e6)
        b.sync()
    bursts = []
    for _ in range(1000):
        t0 = time.perf_counter()
        for _ in range(16):
            fill(h, None)
        bursts.append((time.perf_counter() - t0) / 16 * 1e6)
        b.sync()
    single = []
    for _ in range(2000):
        t0 = time.perf_counter()
        fill(h, None)
        b.sync()
        single.append((time.perf_counter() - t0) * 1e6)
    print(json.dumps({"lib": os.environ.get("DPX_LIB", ""), "kernel": b.describe()["kernel"], "enqueue_us": round(statistics.median(rounds), 3),
                      "enqueue_us_rounds": [round(x, 3) for x in rounds], "burst_us": round(statistics.median(bursts), 3),
                      "fill_sync_us": round(statistics.median(single), 3)}))
