#!/usr/bin/env python3
"""A/B of the table fill of local band-direction batches (dpx_batch_set_local_direction_table, k_bdlt_fill) against the plain fill of the
same batch (k_bdl_fill), after tools/bdl_ab.py's method: per workload and algorithm ONE DPX_KEEP_LOCAL_BAND_DIRECTIONS batch, on which a
table equivalent to the batch's match / mismatch is set and cleared in turn
    TABLE  k_bdlt_fill (the identity-equivalent table: the same cells, the same codes, the same stores)
    PLAIN  k_bdl_fill
alternating (--reps times each, the order swapped every rep; one discarded warm-up fill, then --fills timed fills per measurement,
dpx_batch_fill_timed).  Every child asserts that both modes give the same scores and end cells.  Workloads: --pairs x 4096^2 at band 128
(related, 8 % substitutions and a planted 60-base deletion), --short-reads short reads at band 64, and --long-pairs pairs of
30 000 x 30 000 at band 256.

--plain-only measures PLAIN alone and --package DIR imports the package from DIR instead of this tree: together they time the plain
fills of another build (the parent commit's package and library, say) in the same job.

The parent process starts --processes fresh child processes one after the other (it never opens the GPU itself), each under its own
time limit, stops at the first child that fails, and prints, per workload, algorithm and mode, the median [min, max] of the children's
medians.  Needs a GPU.  A measurement tool: it is not run as a test and gates nothing."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = (3, -1, -3, -1)  # BSW: one gap weight of -3
MODES = ("TABLE", "PLAIN")


def identity_table():
    """match / mismatch of W over the letters of the workloads' texts (ACGT, and 0123 in the short reads) as a 9 x 9 table; every other
    byte takes the ninth code, which no text uses"""
    letters = b"ACGT0123"
    tab = np.full((len(letters) + 1,) * 2, W[1], np.int8)
    np.fill_diagonal(tab, W[0])
    code = np.full(256, len(letters), np.uint8)
    for k, ch in enumerate(letters):
        code[ch] = k
    return tab, code


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
    table = identity_table()

    def measure(b, name, algo, mode, band):
        if not args.plain_only:
            b.set_local_direction_table(*(table if mode == "TABLE" else (None,)))
        b.fill_timed(1)  # warm-up (code load, the table's upload): discarded
        us = b.fill_timed(args.fills)
        d = b.describe()
        assert d["kernel"] == ("k_bdlt_fill" if mode == "TABLE" else "k_bdl_fill"), d
        print(json.dumps({"workload": name, "algo": algo, "mode": mode, "band": band, "kernel": d["kernel"], "cells_per_lane": d["rows_per_lane"],
                          "waves_per_workgroup": d["waves_per_workgroup"], "fill_us": round(us, 1)}), flush=True)
        return [x.copy() for x in b.results()]

    work = [(f"{args.pairs} x 4096^2 related", related(args.pairs, 4096, 43), args.band),
            (f"{args.short_reads} short reads", make_ragged_batch(args.short_reads, 80, 130, 100, 160, seed=44), 64)]
    if args.long_pairs:
        work.append((f"{args.long_pairs} x 30000^2", related(args.long_pairs, 30000, 47, gap=150), 256))
    for name, sb, band in work:
        assert set(np.unique(sb.sequences).tolist()) <= set(b"\0ACGT0123456789"), name  # the table's letters (and the pair numbers between the strings)
        for algo, code in (("BSW", dpx.ALGO_BSW), ("BASW", dpx.ALGO_BASW)):
            w = W if algo == "BASW" else W[:3] + (0,)
            with dpx.Batch(code, sb.sequences, sb.pairs, *w, band=band, flags=dpx.KEEP_LOCAL_BAND_DIRECTIONS) as b:
                seen = {}
                for rep in range(args.reps):
                    for mode in (("PLAIN",) if args.plain_only else MODES if rep % 2 == 0 else MODES[::-1]):
                        got = measure(b, name, algo, mode, band)
                        seen.setdefault(mode, got)
                        for x, y in zip(got, seen["PLAIN" if "PLAIN" in seen else mode]):  # both modes, every repetition: the same results
                            assert np.array_equal(x, y), (name, algo, mode, rep)
                assert args.plain_only or set(seen) == set(MODES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--fills", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--band", type=int, default=128)
    ap.add_argument("--short-reads", type=int, default=100000)
    ap.add_argument("--long-pairs", type=int, default=256)
    ap.add_argument("--plain-only", action="store_true", help="time k_bdl_fill alone (a build without the setter)")
    ap.add_argument("--package", default=ROOT, help="directory that holds the dpx_gpu_genomics_project_amd package to measure")
    ap.add_argument("--child-timeout", type=float, default=300.0, help="seconds after which a child process is killed")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package))
    if args.child:
        return child(args)
    recs = []
    for proc in range(args.processes):  # one after the other, each under its own limit; the first failure ends the run
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"],
                              capture_output=True, text=True, timeout=args.child_timeout)  # (a hung fill must not hold the card)
        if done.returncode != 0:
            sys.stderr.write(done.stderr[-4000:])
            raise SystemExit(f"child {proc} ended with status {done.returncode}: nothing more is started")
        for line in done.stdout.splitlines():
            rec = json.loads(line)
            rec["process"] = proc
            print(json.dumps(rec), flush=True)
            recs.append(rec)
    print(f"summary, package {os.path.relpath(os.path.abspath(args.package), ROOT)}, weights {W}: fill time, median [min, max] over {args.processes} fresh "
          f"processes of each process's median ({args.reps} measurements of {args.fills} fills); both modes gave equal results in every child")
    for name, algo in dict.fromkeys((r["workload"], r["algo"]) for r in recs):
        base = None
        for mode in MODES[::-1]:
            mine = [r for r in recs if (r["workload"], r["algo"], r["mode"]) == (name, algo, mode)]
            per = [statistics.median([r["fill_us"] for r in mine if r["process"] == p]) for p in range(args.processes) if any(r["process"] == p for r in mine)]
            if not per:
                continue
            med = statistics.median(per)
            base = med if mode == "PLAIN" else base
            print(f"  {name:28s} {algo:4s} {mode:5s} {mine[0]['kernel']:12s} band {mine[0]['band']:3d} C {mine[0]['cells_per_lane']} wpb {mine[0]['waves_per_workgroup']} "
                  f"{med / 1e3:9.3f} ms [{min(per) / 1e3:.3f}, {max(per) / 1e3:.3f}]" + (f"  x{med / base:.3f} of the plain fill" if base and mode != "PLAIN" else ""))


if __name__ == "__main__":
    main()
