#!/usr/bin/env python3
"""A/B of DPX_ALGO_ASG against DPX_ALGO_ANW and DPX_ALGO_ASW on the same seeded pairs, alternating the three (--reps times each, in one
process, the order reversed every other rep; every batch runs one discarded warm-up fill first): fill GCUPS (hipEvents, fill_timed), output time (traceback + text to
the host, wall clock around output_begin / output_end), for 1000 x 1024^2 with matrices and with directions, and 100 000 short reads
(reference 100-160, query 80-130); then dpx_main end to end on a 1000 x 1024^2 file.  One JSON line per measurement, then a summary
(median [min, max]).  Needs a GPU."""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dpx_gpu_genomics_project_amd as dpx  # noqa: E402
from dpx_gpu_genomics_project_amd.synth import make_batch, make_ragged_batch, write_pairs_file  # noqa: E402

W = (3, -1, -3, -1)
ALGOS = {"ANW": dpx.ALGO_ANW, "ASW": dpx.ALGO_ASW, "ASG": dpx.ALGO_ASG}


def one(name, algo, sb, fills, flags=dpx.KEEP_MATRICES):
    with dpx.Batch(ALGOS[algo], sb.sequences, sb.pairs, *W, flags=flags | dpx.TIME_FILLS) as b:
        b.fill_timed(1)  # warm-up (first touch of the pool, code load): discarded
        us = b.fill_timed(fills)
        t0 = time.perf_counter()
        b.output_begin(0)
        text, _ = b.output_end()
        out_ms = (time.perf_counter() - t0) * 1e3
        rec = {"workload": name, "algo": algo, "fill_us": round(us, 1), "gcups": round(sb.cells / us / 1e3, 1), "output_ms": round(out_ms, 3),
               "matrix_bytes": b.info()["matrix_bytes"], "text_bytes": len(text), "kernel": b.describe()["kernel"]}
    print(json.dumps(rec), flush=True)
    return rec


def driver(path, algo):
    cmd = [os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "hostcpp", "dpx_main"), "-pairs", path, "-match", "3", "-mismatch", "-1", "-open", "-3",
           "-extend", "-1", "-algo", algo]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"dpx_main failed ({r.returncode}): {r.stderr[-500:]!r}")
    out = r.stdout.decode("latin-1")
    us = float(re.search(r"Elapsed time \(usec\): (\d+(?:\.\d+)?)", out).group(1))
    rec = {"workload": "dpx_main 1000 x 1024^2", "algo": algo, "elapsed_ms": round(us / 1e3, 3), "stdout_bytes": len(out)}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fills", type=int, default=5)
    ap.add_argument("--no-driver", action="store_true")
    args = ap.parse_args()
    dpx.init(0)
    long_pairs = make_batch(1000, 1024, 1024, seed=43)
    work = [("1000 x 1024^2", long_pairs, dpx.KEEP_MATRICES), ("1000 x 1024^2 directions", long_pairs, dpx.KEEP_DIRECTIONS),
            ("100000 short reads", make_ragged_batch(100000, 80, 130, 100, 160, seed=44), dpx.KEEP_MATRICES)]
    recs = []
    for name, sb, flags in work:
        for rep in range(args.reps):
            for algo in (list(ALGOS) if rep % 2 == 0 else list(ALGOS)[::-1]):
                recs.append(one(name, algo, sb, args.fills, flags))
    if not args.no_driver:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "long.txt")
            write_pairs_file(make_batch(1000, 1024, 1024, seed=45), path)
            for rep in range(args.reps):
                for algo in (list(ALGOS) if rep % 2 == 0 else list(ALGOS)[::-1]):
                    recs.append(driver(path, algo))
    print("summary (median [min, max]):")
    for wl, algo in sorted({(r["workload"], r["algo"]) for r in recs}):
        rs = [r for r in recs if r["workload"] == wl and r["algo"] == algo]
        fields = ["elapsed_ms"] if "elapsed_ms" in rs[0] else ["gcups", "output_ms", "matrix_bytes"]
        txt = ", ".join(f"{f} {statistics.median(r[f] for r in rs):g} [{min(r[f] for r in rs):g}, {max(r[f] for r in rs):g}]" for f in fields)
        print(f"  {wl:24s} {algo:4s} {txt}")


if __name__ == "__main__":
    main()
