#!/usr/bin/env python3
"""A/B of two-piece local band-direction batches (DPX_LOCAL_TWO_PIECE_GAPS, k_lb2_fill) after tools/bd2_ab.py's and tools/bdl_ab.py's
method: the same seeded pairs as ONE one-piece BASW batch and ONE two-piece batch per workload, both alive, filled in turn
    ONE  k_bdl_fill (under the table: k_bdlt_fill), 4-bit codes
    TWO  k_lb2_fill, 8-bit codes
alternating (--reps times each, the order swapped every rep; one discarded warm-up fill, then --fills timed fills per measurement,
dpx_batch_fill_timed), and once per batch and setting the wall time of traceback + text (dpx_batch_output_begin / _end).  Settings: piece 2
equal to piece 1 and (-4, -2 / -24, -1), each without and with the 5 x 5 ACGTN table; the one-piece batch always scores by piece 1.
Workloads: --pairs x 4096^2 at band 128 (related, 8 % substitutions and a planted 60-base deletion), --short-reads short reads at band 64,
and --long-pairs pairs of 30 000 x 30 000 at band 256.  Equal results are asserted in every child: with equal pieces the two batches
report the same scores, end cells and text; with unequal pieces no two-piece score is below the one-piece score.

The parent process starts --processes fresh child processes one after the other (it never opens the GPU itself), each under its own time
limit, and prints, per workload and setting, the median [min, max] of the children's medians and the pool bytes.  Needs a GPU.  A
measurement tool: it is not run as a test and gates nothing."""
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
MODES = ("ONE", "TWO")
SETTINGS = [("equal", P1, False), ("equal+table", P1, True), ("two-piece", P2, False), ("two-piece+table", P2, True)]


def acgtn_table():
    """(2, -3) among ACGT, the N row and column -1; lower case folds, every other byte is N"""
    scores = np.full((5, 5), -3, np.int8)
    np.fill_diagonal(scores, 2)
    scores[4, :] = -1
    scores[:, 4] = -1
    code = np.full(256, 4, np.uint8)
    for k, ch in enumerate(b"ACGT"):
        code[ch] = code[ch + 32] = k
    return scores, code


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
    table = acgtn_table()

    def measure(b, name, setting, mode, band):
        b.fill_timed(1)  # warm-up (first touch of the pool, code load): discarded
        us = b.fill_timed(args.fills)
        d = b.describe()
        print(json.dumps({"workload": name, "setting": setting, "mode": mode, "band": band, "kernel": d["kernel"], "cells_per_lane": d["rows_per_lane"],
                          "waves_per_workgroup": d["waves_per_workgroup"], "fill_us": round(us, 1), "pool_bytes": b.info()["matrix_bytes"]}), flush=True)

    def text(b, name, setting, mode):
        b.fill()
        b.sync()
        t0 = time.perf_counter()
        b.output_begin(0)
        out, _ = b.output_end()
        print(json.dumps({"workload": name, "setting": setting, "mode": mode + "_TEXT", "wall_us": round((time.perf_counter() - t0) * 1e6, 1), "text_bytes": len(out)}), flush=True)
        return out

    work = [(f"{args.pairs} x 4096^2 related", related(args.pairs, 4096, 43), args.band),
            (f"{args.short_reads} short reads", make_ragged_batch(args.short_reads, 80, 130, 100, 160, seed=44), 64)]
    if args.long_pairs:
        work.append((f"{args.long_pairs} x 30000^2", related(args.long_pairs, 30000, 47, gap=150), 256))
    for name, sb, band in work:
        with dpx.Batch(dpx.ALGO_BASW, sb.sequences, sb.pairs, *MM, *P1, band=band, flags=dpx.KEEP_LOCAL_BAND_DIRECTIONS) as one, \
             dpx.Batch(dpx.ALGO_BASW, sb.sequences, sb.pairs, *MM, *P1, band=band, flags=dpx.KEEP_LOCAL_BAND_DIRECTIONS | dpx.LOCAL_TWO_PIECE_GAPS) as two:
            for setting, piece2, tabled in SETTINGS:
                two.set_second_gap(*piece2)
                for b in (one, two):
                    b.set_local_direction_table(*(table if tabled else (None,)))
                assert one.describe()["kernel"] == ("k_bdlt_fill" if tabled else "k_bdl_fill") and two.describe()["kernel"] == "k_lb2_fill"
                for rep in range(args.reps):
                    for mode in (MODES if rep % 2 == 0 else MODES[::-1]):
                        measure(two if mode == "TWO" else one, name, setting, mode, band)
                texts = [text(one, name, setting, "ONE"), text(two, name, setting, "TWO")]
                (s1, r1, c1), (s2, r2, c2) = one.results(), two.results()
                if piece2 == P1:
                    assert np.array_equal(s1, s2) and np.array_equal(r1, r2) and np.array_equal(c1, c2) and texts[0] == texts[1], (name, setting)
                else:
                    assert np.all(s2 >= s1), (name, setting)  # (a second piece only adds paths)
                    print(json.dumps({"workload": name, "setting": setting, "mode": "GAIN", "pairs_above_one_piece": int((s2 > s1).sum()), "pairs": int(len(s1))}), flush=True)


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
    print(f"summary, match / mismatch {MM}, piece 1 {P1}, piece 2 {P2} where it differs: fill time, median [min, max] over {args.processes} fresh processes of each "
          f"process's median ({args.reps} measurements of {args.fills} fills); traceback + text: wall time, one per process")
    for name, setting in dict.fromkeys((r["workload"], r["setting"]) for r in recs):
        base = None
        for mode in MODES:
            mine = [r for r in recs if (r["workload"], r["setting"], r["mode"]) == (name, setting, mode)]
            per = [statistics.median([r["fill_us"] for r in mine if r["process"] == p]) for p in range(args.processes) if any(r["process"] == p for r in mine)]
            if not per:
                continue
            med = statistics.median(per)
            base = med if mode == "ONE" else base
            walls = [r["wall_us"] for r in recs if (r["workload"], r["setting"], r["mode"]) == (name, setting, mode + "_TEXT")]
            print(f"  {name:28s} {setting:16s} {mode:3s} {mine[0]['kernel']:12s} band {mine[0]['band']:3d} wpb {mine[0]['waves_per_workgroup']} {med / 1e3:9.3f} ms "
                  f"[{min(per) / 1e3:.3f}, {max(per) / 1e3:.3f}]  pool {mine[0]['pool_bytes']:>12d} B"
                  + (f"  x{med / base:.3f} of the one-piece fill" if base and mode != "ONE" else "")
                  + (f"  traceback + text {statistics.median(walls) / 1e3:.3f} ms [{min(walls) / 1e3:.3f}, {max(walls) / 1e3:.3f}]" if walls else ""))
        gains = [r for r in recs if (r["workload"], r["setting"], r["mode"]) == (name, setting, "GAIN")]
        if gains:
            print(f"  {name:28s} {setting:16s} the two-piece score is above the one-piece score on {gains[0]['pairs_above_one_piece']} of {gains[0]['pairs']} pairs")


if __name__ == "__main__":
    main()
