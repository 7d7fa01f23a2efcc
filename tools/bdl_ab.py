#!/usr/bin/env python3
"""A/B of local band-direction batches (DPX_KEEP_LOCAL_BAND_DIRECTIONS, k_bdl_fill) after tools/bd2_ab.py's method: the same seeded pairs as
ONE int16 matrix batch and ONE direction batch per workload and algorithm, both alive, filled in turn
    MATRIX      k_banded_fill / k_banded_fill_pk (BSW), k_basw_fill (BASW)
    DIRECTIONS  k_bdl_fill
alternating (--reps times each, the order swapped every rep; one discarded warm-up fill, then --fills timed fills per measurement,
dpx_batch_fill_timed), and once per batch the wall time of traceback + text (dpx_batch_output_begin / _end).  Workloads: --pairs x 4096^2
at band 128 (related, 8 % substitutions and a planted 60-base deletion), --short-reads short reads at band 64, and --long-pairs pairs of
30 000 x 30 000 at band 256, which only the direction batch admits (the matrix batch answers DPX_ERR_RANGE; that is asserted).

The parent process starts --processes fresh child processes one after the other (it never opens the GPU itself) and prints, per workload,
algorithm and mode, the median [min, max] of the children's medians and the pool bytes.  Needs a GPU.  A measurement tool: it is not run
as a test and gates nothing."""
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

W = (3, -1, -3, -1)  # BSW: one gap weight of -3
MODES = ("MATRIX", "DIRECTIONS")


def related(count, size, seed, gap=60):
    """`count` pairs: the query is the reference of `size` bases with 8 % substitutions and one deletion of `gap` bases in the middle"""
    from dpx_gpu_genomics_project_amd.synth import from_strings

    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    texts = []
    for _ in range(count):
        ref = rng.integers(0, 4, size)
        q = ref.copy()
        sub = rng.random(size) < 0.08
        q[sub] = rng.integers(0, 4, int(sub.sum()))
        q = np.concatenate([q[:size // 2], q[size // 2 + gap:]])
        texts.append((acgt[ref].tobytes(), acgt[q].tobytes()))
    return from_strings(texts)


def child(args):
    import dpx_gpu_genomics_project_amd as dpx
    from dpx_gpu_genomics_project_amd.synth import make_ragged_batch

    dpx.init(0)

    def measure(b, name, algo, mode, band):
        b.fill_timed(1)  # warm-up (first touch of the pool, code load): discarded
        us = b.fill_timed(args.fills)
        d = b.describe()
        print(json.dumps({"workload": name, "algo": algo, "mode": mode, "band": band, "kernel": d["kernel"], "cells_per_lane": d["rows_per_lane"],
                          "waves_per_workgroup": d["waves_per_workgroup"], "fill_us": round(us, 1), "pool_bytes": b.info()["matrix_bytes"]}), flush=True)

    def text(b, name, algo, mode):
        b.fill()
        b.sync()
        t0 = time.perf_counter()
        b.output_begin(0)
        out, _ = b.output_end()
        print(json.dumps({"workload": name, "algo": algo, "mode": mode + "_TEXT", "wall_us": round((time.perf_counter() - t0) * 1e6, 1), "text_bytes": len(out)}), flush=True)

    work = [(f"{args.pairs} x 4096^2 related", related(args.pairs, 4096, 43), args.band, True),
            (f"{args.short_reads} short reads", make_ragged_batch(args.short_reads, 80, 130, 100, 160, seed=44), 64, True)]
    if args.long_pairs:
        work.append((f"{args.long_pairs} x 30000^2", related(args.long_pairs, 30000, 47, gap=150), 256, False))
    for name, sb, band, admitted in work:
        for algo, code in (("BSW", dpx.ALGO_BSW), ("BASW", dpx.ALGO_BASW)):
            w = W if algo == "BASW" else W[:3] + (0,)
            with dpx.Batch(code, sb.sequences, sb.pairs, *w, band=band, flags=dpx.KEEP_LOCAL_BAND_DIRECTIONS) as dirs:
                if not admitted:
                    try:
                        dpx.Batch(code, sb.sequences, sb.pairs, *w, band=band)
                        raise SystemExit("the matrix batch admitted the long pairs")
                    except dpx.DpxError as e:
                        assert e.status == -4, e.status  # DPX_ERR_RANGE
                    for _ in range(args.reps):
                        measure(dirs, name, algo, "DIRECTIONS", band)
                    text(dirs, name, algo, "DIRECTIONS")
                    continue
                with dpx.Batch(code, sb.sequences, sb.pairs, *w, band=band) as mat:
                    for rep in range(args.reps):
                        for mode in (MODES if rep % 2 == 0 else MODES[::-1]):
                            measure(dirs if mode == "DIRECTIONS" else mat, name, algo, mode, band)
                    text(mat, name, algo, "MATRIX")
                    text(dirs, name, algo, "DIRECTIONS")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--fills", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--band", type=int, default=128)
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
    print(f"summary, weights {W}: fill time, median [min, max] over {args.processes} fresh processes of each process's median "
          f"({args.reps} measurements of {args.fills} fills); traceback + text: wall time, one per process")
    for name, algo in dict.fromkeys((r["workload"], r["algo"]) for r in recs):
        base = None
        for mode in MODES:
            mine = [r for r in recs if (r["workload"], r["algo"], r["mode"]) == (name, algo, mode)]
            per = [statistics.median([r["fill_us"] for r in mine if r["process"] == p]) for p in range(args.processes) if any(r["process"] == p for r in mine)]
            if not per:
                continue
            med = statistics.median(per)
            base = med if mode == "MATRIX" else base
            walls = [r["wall_us"] for r in recs if (r["workload"], r["algo"], r["mode"]) == (name, algo, mode + "_TEXT")]
            print(f"  {name:28s} {algo:4s} {mode:10s} {mine[0]['kernel']:16s} band {mine[0]['band']:3d} wpb {mine[0]['waves_per_workgroup']} {med / 1e3:9.3f} ms "
                  f"[{min(per) / 1e3:.3f}, {max(per) / 1e3:.3f}]  pool {mine[0]['pool_bytes']:>12d} B"
                  + (f"  x{med / base:.3f} of the matrix fill" if base and mode != "MATRIX" else "")
                  + (f"  traceback + text {statistics.median(walls) / 1e3:.3f} ms [{min(walls) / 1e3:.3f}, {max(walls) / 1e3:.3f}]" if walls else ""))


if __name__ == "__main__":
    main()
