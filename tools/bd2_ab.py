#!/usr/bin/env python3
"""A/B of two-piece band-direction batches (DPX_TWO_PIECE_GAPS, k_bd2_fill) after tools/bdx_ab.py's method: the same seeded pairs as ONE
unflagged band-direction BAXT batch and ONE two-piece batch per workload, both alive, filled in turn as
    BDIR            k_bdir_fill (the unflagged batch, nothing on)
    BD2_EQUAL       k_bd2_fill with the second piece equal to the first
    BD2_TWO         k_bd2_fill with (-4, -2 / -24, -1)
    BDX_TABLE_DROP  k_bdx_fill under table + z-drop (the unflagged batch)
    BD2_TABLE_DROP  k_bd2_fill under table + z-drop with the two pieces
the modes alternating (--reps times each, the order rotated every rep; one discarded warm-up fill, then --fills timed fills per
measurement, dpx_batch_fill_timed).  The table is the identity-equivalent one; Z = --zdrop, E = 5.  Workloads: --pairs x 4096^2 at band 128
(related, with a planted 60-base deletion), --short-reads short reads, and --long-pairs pairs of 30 000 x 30 000 at band 256, for which the
time of traceback and text of the two-piece batch is taken too.

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

MM, P1, P2 = (2, -4), (-4, -2), (-24, -1)
E = 5
MODES = ("BDIR", "BD2_EQUAL", "BD2_TWO", "BDX_TABLE_DROP", "BD2_TABLE_DROP")


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

    def measure(b, name, mode, band):
        b.fill_timed(1)  # warm-up (first touch of the pool, code load): discarded
        us = b.fill_timed(args.fills)
        d = b.describe()
        print(json.dumps({"workload": name, "mode": mode, "band": band, "kernel": d["kernel"], "cells_per_lane": d["rows_per_lane"],
                          "waves_per_workgroup": d["waves_per_workgroup"], "fill_us": round(us, 1), "pool_bytes": b.info()["matrix_bytes"]}), flush=True)

    work = [(f"{args.pairs} x 4096^2 related", related(args.pairs, 4096, 43), b"ACGT", args.band, False),
            (f"{args.short_reads} short reads", make_ragged_batch(args.short_reads, 80, 130, 100, 160, seed=44), b"0123", args.band, False)]
    if args.long_pairs:
        work.append((f"{args.long_pairs} x 30000^2", related(args.long_pairs, 30000, 47, gap=150), b"ACGT", 256, True))
    for name, sb, letters, band, text in work:
        table = np.full((4, 4), MM[1], np.int8)
        np.fill_diagonal(table, MM[0])
        code = dpx.code_table(letters)
        with dpx.Batch(dpx.ALGO_BAXT, sb.sequences, sb.pairs, *MM, *P1, band=band, flags=dpx.KEEP_BAND_DIRECTIONS) as one, \
                dpx.Batch(dpx.ALGO_BAXT, sb.sequences, sb.pairs, *MM, *P1, band=band, flags=dpx.KEEP_BAND_DIRECTIONS | dpx.TWO_PIECE_GAPS) as two:
            for rep in range(args.reps):
                k = rep % len(MODES)
                for mode in MODES[k:] + MODES[:k]:
                    b = two if mode.startswith("BD2") else one
                    if b is two:
                        b.set_second_gap(*(P1 if mode == "BD2_EQUAL" else P2))
                    if mode.endswith("TABLE_DROP"):
                        b.set_direction_scoring(args.zdrop, E, table, code)
                    else:
                        b.set_direction_scoring(-1, -1, None, None)
                    measure(b, name, mode, band)
            if text:
                two.fill()
                t0 = time.perf_counter()
                two.output_begin(0)
                out, _ = two.output_end()
                print(json.dumps({"workload": name, "mode": "TRACEBACK_TEXT", "wall_us": round((time.perf_counter() - t0) * 1e6, 1),
                                  "text_bytes": len(out)}), flush=True)


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
    print(f"summary, pieces {P1} / {P2}, Z = {args.zdrop}, E = {E}: fill time, median [min, max] over {args.processes} fresh processes of each "
          f"process's median ({args.reps} measurements of {args.fills} fills)")
    for name in dict.fromkeys(r["workload"] for r in recs):
        base = None
        for mode in MODES:
            per = [statistics.median([r["fill_us"] for r in recs if (r["workload"], r["mode"], r["process"]) == (name, mode, p)])
                   for p in range(args.processes) if any((r["workload"], r["mode"], r["process"]) == (name, mode, p) for r in recs)]
            if not per:
                continue
            first = next(r for r in recs if r["workload"] == name and r["mode"] == mode)
            med = statistics.median(per)
            base = med if mode == "BDIR" else base
            print(f"  {name:32s} {mode:15s} {first['kernel']:12s} band {first['band']:3d} wpb {first['waves_per_workgroup']} {med / 1e3:9.3f} ms "
                  f"[{min(per) / 1e3:.3f}, {max(per) / 1e3:.3f}]  pool {first['pool_bytes']}" + (f"  x{med / base:.3f} of k_bdir_fill" if base else ""))
        walls = [r["wall_us"] for r in recs if r["workload"] == name and r["mode"] == "TRACEBACK_TEXT"]
        if walls:
            print(f"  {name:32s} traceback + text (wall) {statistics.median(walls) / 1e3:9.3f} ms [{min(walls) / 1e3:.3f}, {max(walls) / 1e3:.3f}]")


if __name__ == "__main__":
    main()
