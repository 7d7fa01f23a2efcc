#!/usr/bin/env python3
"""A/B of DPX_KEEP_MATRICES against DPX_KEEP_DIRECTIONS batches of the same pairs, alternating the two modes (--reps times each, in one process):
fill GCUPS (hipEvents, fill_timed), output time (traceback + text to the host, wall clock around output_begin / output_end) and pool bytes,
for LSW 10 000 x 1024^2, ANW 1 000 x 1024^2 and 100 000 short reads (LNW); then dpx_main end to end on a 10 000 x 1024^2 file with and
without -directions.  One JSON line per measurement, then a summary (median [min, max]) per workload and mode.  Needs a GPU."""
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

W = {dpx.ALGO_LNW: (3, -1, -2, -1), dpx.ALGO_LSW: (3, -1, -2, -1), dpx.ALGO_ANW: (3, -1, -3, -1)}
MODES = {"matrices": dpx.KEEP_MATRICES, "directions": dpx.KEEP_DIRECTIONS}


def one(name, algo, sb, mode, fills):
    with dpx.Batch(algo, sb.sequences, sb.pairs, *W[algo], flags=MODES[mode] | dpx.TIME_FILLS) as b:
        us = b.fill_timed(fills)
        t0 = time.perf_counter()
        b.output_begin(0)
        text, _ = b.output_end()
        out_ms = (time.perf_counter() - t0) * 1e3
        rec = {"workload": name, "mode": mode, "fill_us": round(us, 1), "gcups": round(sb.cells / us / 1e3, 1), "output_ms": round(out_ms, 3),
               "matrix_bytes": b.info()["matrix_bytes"], "text_bytes": len(text), "kernel": b.describe()["kernel"]}
    print(json.dumps(rec), flush=True)
    return rec


def driver(path, directions, algo="LSW"):
    cmd = [os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "hostcpp", "dpx_main"), "-pairs", path, "-match", "3", "-mismatch", "-1", "-open", "-2",
           "-algo", algo] + (["-directions"] if directions else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0:
        raise SystemExit(f"dpx_main failed ({r.returncode}): {r.stderr[-500:]!r}")
    out = r.stdout.decode("latin-1")
    us = float(re.search(r"Elapsed time \(usec\): (\d+(?:\.\d+)?)", out).group(1))
    rec = {"workload": "dpx_main LSW 10000 x 1024^2", "mode": "directions" if directions else "matrices", "elapsed_ms": round(us / 1e3, 3),
           "stdout_bytes": len(out)}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fills", type=int, default=5)
    ap.add_argument("--no-driver", action="store_true")
    args = ap.parse_args()
    dpx.init(0)
    work = [("LSW 10000 x 1024^2", dpx.ALGO_LSW, make_batch(10000, 1024, 1024, seed=42)),
            ("ANW 1000 x 1024^2", dpx.ALGO_ANW, make_batch(1000, 1024, 1024, seed=43)),
            ("LNW 100000 short reads", dpx.ALGO_LNW, make_ragged_batch(100000, 80, 130, 100, 160, seed=44))]
    recs = []
    for name, algo, sb in work:
        for _ in range(args.reps):
            for mode in MODES:
                recs.append(one(name, algo, sb, mode, args.fills))
    if not args.no_driver:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "long.txt")
            write_pairs_file(make_batch(10000, 1024, 1024, seed=45), path)
            for _ in range(args.reps):
                for directions in (False, True):
                    recs.append(driver(path, directions))
    print("summary (median [min, max]):")
    keys = sorted({(r["workload"], r["mode"]) for r in recs})
    for wl, mode in keys:
        rs = [r for r in recs if r["workload"] == wl and r["mode"] == mode]
        fields = ["elapsed_ms"] if "elapsed_ms" in rs[0] else ["gcups", "output_ms", "matrix_bytes"]
        txt = ", ".join(f"{f} {statistics.median(r[f] for r in rs):g} [{min(r[f] for r in rs):g}, {max(r[f] for r in rs):g}]" for f in fields)
        print(f"  {wl:28s} {mode:10s} {txt}")


if __name__ == "__main__":
    main()
