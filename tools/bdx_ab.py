#!/usr/bin/env python3
"""A/B of band-direction batches under dpx_batch_set_direction_scoring (k_bdx_fill) after tools/zsub_ab.py's method: the same seeded pairs
on ONE band-direction BAXT batch per workload, filled as plain k_bdir_fill<EXT> and in the five BAXT modes of k_bdx_fill (table, end
bonus, z-drop, table + end bonus, table + z-drop), the modes alternating (--reps times each, the order rotated every rep; one discarded
warm-up fill, then --fills timed fills per measurement, dpx_batch_fill_timed); and the same pairs as a matrix batch under k_zsub_fill
(int16 cells and three planes against int32 cells and one code per cell).  The table is the identity-equivalent one, so every mode
computes the same cells; Z = --zdrop.  Workloads: --pairs x 4096^2 at band 128 fully related (nothing drops at Z = 400) and related for the
first 1024 bases only (the pairs drop; the mean lastDiag is printed), and --short-reads short reads.  Then one workload the matrix batch
refuses: --long-pairs pairs of 30 000 x 30 000 at band 256 with table, Z and E: fill time, the time of traceback and text, pool bytes.

The parent process starts --processes fresh child processes one after the other (it never opens the GPU itself) and prints, per workload
and mode, the median [min, max] of the children's medians.  Needs a GPU.  A measurement tool: it is not run as a test and gates nothing."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = (2, -3, -5, -1)
E = 5
MODES = ("BDIR", "TABLE", "BONUS", "DROP", "TABLE_BONUS", "TABLE_DROP")


def related(count, size, shared, seed):
    """`count` pairs of `size` bases: the query copies the reference's first `shared` bases with 8 % substitutions, the rest is random"""
    from dpx_gpu_genomics_project_amd.synth import from_strings

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


def identity(dpx, letters):
    table = np.full((4, 4), W[1], np.int8)
    np.fill_diagonal(table, W[0])
    return table, dpx.code_table(letters)


def set_mode(b, mode, zdrop, table, code):
    with_table = mode.startswith("TABLE")
    z = zdrop if mode.endswith("DROP") else -1
    e = E if mode.endswith(("BONUS", "DROP")) else -1
    b.set_direction_scoring(z, e, table if with_table else None, code if with_table else None)


def child(args):
    import dpx_gpu_genomics_project_amd as dpx
    from dpx_gpu_genomics_project_amd.synth import make_ragged_batch

    dpx.init(0)

    def measure(b, name, mode, band, scan):
        b.fill_timed(1)  # warm-up (first touch of the pool, code load): discarded
        us = b.fill_timed(args.fills)
        d = b.describe()
        rec = {"workload": name, "mode": mode, "band": band, "kernel": d["kernel"], "cells_per_lane": d["rows_per_lane"],
               "waves_per_workgroup": d["waves_per_workgroup"], "fill_us": round(us, 1), "pool_bytes": b.info()["matrix_bytes"]}
        if scan:
            ext = b.extensions()
            rec["dropped"] = int(np.sum((ext["flags"] & dpx.EXT_ZDROPPED) != 0))
            rec["mean_last_diag"] = round(float(np.mean(ext["lastDiag"])), 1)
        print(json.dumps(rec), flush=True)

    work = [(f"{args.pairs} x 4096^2 related", related(args.pairs, 4096, 4096, 43), b"ACGT"),
            (f"{args.pairs} x 4096^2 related for 1024", related(args.pairs, 4096, 1024, 45), b"ACGT"),
            (f"{args.short_reads} short reads", make_ragged_batch(args.short_reads, 80, 130, 100, 160, seed=44), b"0123")]
    for name, sb, letters in work:
        table, code = identity(dpx, letters)
        with dpx.Batch(dpx.ALGO_BAXT, sb.sequences, sb.pairs, *W, band=args.band, flags=dpx.KEEP_BAND_DIRECTIONS) as b:
            for rep in range(args.reps):
                k = rep % len(MODES)
                for mode in MODES[k:] + MODES[:k]:
                    set_mode(b, mode, args.zdrop, table, code)
                    measure(b, name, mode, args.band, mode.endswith(("BONUS", "DROP")))
        with dpx.Batch(dpx.ALGO_BAXT, sb.sequences, sb.pairs, *W, band=args.band) as mb:  # the matrix batch: k_zsub_fill
            mb.set_extension_table(args.zdrop, E, table, code)
            for rep in range(args.reps):
                measure(mb, name, "MATRIX_ZSUB", args.band, True)
    if args.long_pairs:
        sb = related(args.long_pairs, 30000, 28000, 47)
        table, code = identity(dpx, b"ACGT")
        name = f"{args.long_pairs} x 30000^2"
        refused = 0  # the matrix batch refuses these pairs at its creation already (DPX_ERR_RANGE)
        try:
            with dpx.Batch(dpx.ALGO_BAXT, sb.sequences, sb.pairs, *W, band=256) as mb:
                mb.set_extension_table(args.zdrop, E, table, code)
        except dpx.DpxError as e:
            refused = e.status
        with dpx.Batch(dpx.ALGO_BAXT, sb.sequences, sb.pairs, *W, band=256, flags=dpx.KEEP_BAND_DIRECTIONS) as b:
            b.set_direction_scoring(args.zdrop, E, table, code)
            for rep in range(args.reps):
                measure(b, name, "TABLE_DROP", 256, True)
            t0 = time.perf_counter()
            b.output_begin(0)
            text, _ = b.output_end()
            wall = (time.perf_counter() - t0) * 1e6
            print(json.dumps({"workload": name, "mode": "TRACEBACK_TEXT", "wall_us": round(wall, 1), "text_bytes": len(text),
                              "matrix_batch_status": refused}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--fills", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--band", type=int, default=128)
    ap.add_argument("--zdrop", type=int, default=400)
    ap.add_argument("--short-reads", type=int, default=100000)
    ap.add_argument("--long-pairs", type=int, default=256)
    ap.add_argument("--child-timeout", type=float, default=600.0, help="seconds after which a child process is killed")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    recs = []
    for proc in range(args.processes):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"],
                             capture_output=True, text=True, check=True, timeout=args.child_timeout).stdout  # (a hung fill must not hold the card)
        for line in out.splitlines():
            rec = json.loads(line)
            rec["process"] = proc
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    print(f"summary, Z = {args.zdrop}, E = {E}: fill time, median [min, max] over {args.processes} fresh processes of each process's median "
          f"({args.reps} measurements of {args.fills} fills)")
    names = list(dict.fromkeys(r["workload"] for r in recs))
    for name in names:
        base = None
        for mode in MODES + ("MATRIX_ZSUB",):
            per = [statistics.median([r["fill_us"] for r in recs if r["workload"] == name and r["mode"] == mode and r["process"] == p])
                   for p in range(args.processes) if any(r["workload"] == name and r["mode"] == mode and r["process"] == p for r in recs)]
            if not per:
                continue
            first = next(r for r in recs if r["workload"] == name and r["mode"] == mode)
            med = statistics.median(per)
            base = med if mode == "BDIR" else base
            tail = f"  dropped {first['dropped']}, mean lastDiag {first['mean_last_diag']}" if "dropped" in first else ""
            ratio = f"  x{med / base:.3f} of k_bdir_fill" if base else ""
            print(f"  {name:40s} {mode:12s} {first['kernel']:12s} band {first['band']:3d} wpb {first['waves_per_workgroup']} {med / 1e3:9.3f} ms "
                  f"[{min(per) / 1e3:.3f}, {max(per) / 1e3:.3f}]  pool {first['pool_bytes']}{ratio}{tail}")
        for r in recs:
            if r["workload"] == name and r["mode"] == "TRACEBACK_TEXT" and r["process"] == 0:
                walls = [x["wall_us"] for x in recs if x["workload"] == name and x["mode"] == "TRACEBACK_TEXT"]
                print(f"  {name:40s} traceback + text (wall) {statistics.median(walls) / 1e3:9.3f} ms [{min(walls) / 1e3:.3f}, {max(walls) / 1e3:.3f}], "
                      f"{r['text_bytes']} bytes of text; the matrix batch answered status {r['matrix_batch_status']}")


if __name__ == "__main__":
    main()
