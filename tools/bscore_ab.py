#!/usr/bin/env python3
"""A/B of the DPX_LONG_SCORES fills (k_bscore_fill, k_lscore_fill) against the direction batches whose cells they compute (k_bdir_fill /
k_bdx_fill, k_bdl_fill / k_bdlt_fill), after tools/bdl_ab.py's and tools/bdx_ab.py's method: per workload and mode the same pairs go on
    DIR    the band-direction batch (DPX_KEEP_BAND_DIRECTIONS / DPX_KEEP_LOCAL_BAND_DIRECTIONS): what a score-only caller of long pairs runs
           without the flag
    LONG   the same flags | DPX_LONG_SCORES: no pool, nothing stored but the results
    INT16  where the int16 DPX_SCORE_ONLY batch admits the pairs and has the mode (the first two workloads; no table on BSW / BASW): that
           batch, for scale
with the batches' fills alternating (--reps times each, the order swapped every rep; one discarded warm-up fill, then --fills timed
fills per measurement, dpx_batch_fill_timed).  Every child asserts that all sides give the same scores and end cells.  Workloads:
--pairs x 4096^2 at band 128 (related: 8 % substitutions and a planted 60-base deletion), --short-reads short reads at band 64, and
--long-pairs pairs of 30 000 x 30 000 at band 256.  Modes: BANW, BAXT, BAXT under a table with a z-drop that never drops, BAXT under a
table with z-drop on pairs related for their first 1024 bases only (not on the short reads), BSW, BASW, BASW under a table.  The pool
bytes of every side are reported.

--dir-only measures DIR alone and --package DIR imports the package from DIR instead of this tree: together they time the direction
fills of another build (the parent commit's package and library, say) in the same job.

The parent process starts --processes fresh child processes one after the other (it never opens the GPU itself), each under its own
time limit, stops at the first child that fails, and prints, per workload, mode and side, the median [min, max] of the children's
medians.  Needs a GPU.  A measurement tool: it is not run as a test and gates nothing."""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = (2, -4, -4, -2)  # (the int16 batches admit 4096 bases at these)
LONG_SCORES = 0x100
SIDES = ("DIR", "LONG", "INT16")
NEVER = 1 << 20  # a z-drop threshold no pair reaches
# name, algorithm, table?, z-drop (-1 off), pairs related for a prefix only?
MODES = (("BANW", "BANW", False, -1, False), ("BAXT", "BAXT", False, -1, False), ("BAXT table zdrop-never", "BAXT", True, NEVER, False),
         ("BAXT table zdrop prefix-1024", "BAXT", True, 100, True), ("BSW", "BSW", False, -1, False), ("BASW", "BASW", False, -1, False),
         ("BASW table", "BASW", True, -1, False))


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


def related(count, size, seed, gap=60, prefix=0):
    """`count` pairs: the query is the reference of `size` bases with 8 % substitutions and one deletion of `gap` bases in the middle;
    prefix > 0: behind its first `prefix` bases the query is unrelated"""
    from dpx_gpu_genomics_project_amd.synth import from_strings

    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    texts = []
    for _ in range(count):
        ref = rng.integers(0, 4, size)
        q = ref.copy()
        sub = rng.random(size) < 0.08
        q[sub] = rng.integers(0, 4, int(sub.sum()))
        if prefix:
            q[prefix:] = rng.integers(0, 4, size - prefix)
        q = np.concatenate([q[:size // 2], q[size // 2 + gap:]])
        texts.append((acgt[ref].tobytes(), acgt[q].tobytes()))
    return from_strings(texts)


def child(args):
    import dpx_gpu_genomics_project_amd as dpx
    from dpx_gpu_genomics_project_amd.synth import make_ragged_batch

    dpx.init(0)
    table = identity_table()
    codes = {"BANW": dpx.ALGO_BANW, "BAXT": dpx.ALGO_BAXT, "BSW": dpx.ALGO_BSW, "BASW": dpx.ALGO_BASW}

    def make(side, algo, sb, band, with_table, z):
        local = algo in ("BSW", "BASW")
        w = W if algo != "BSW" else W[:3] + (0,)
        storage = dpx.KEEP_LOCAL_BAND_DIRECTIONS if local else dpx.KEEP_BAND_DIRECTIONS
        flags = {"DIR": storage, "LONG": storage | LONG_SCORES, "INT16": dpx.SCORE_ONLY}[side]
        b = dpx.Batch(codes[algo], sb.sequences, sb.pairs, *w, band=band, flags=flags)
        if side == "INT16":
            if with_table and z >= 0:
                b.set_extension_table(z, -1, *table)
            elif with_table:
                b.set_substitution(*table)
            elif z >= 0:
                b.set_extension(z, -1)
        elif local and with_table:
            b.set_local_direction_table(*table)
        elif not local and (with_table or z >= 0):
            b.set_direction_scoring(z, -1, *(table if with_table else (None, None)))
        return b

    def measure(b, name, mode, side, band):
        b.fill_timed(1)  # warm-up (code load): discarded
        us = b.fill_timed(args.fills)
        d = b.describe()
        print(json.dumps({"workload": name, "mode": mode, "side": side, "band": band, "kernel": d["kernel"], "cells_per_lane": d["rows_per_lane"],
                          "waves_per_workgroup": d["waves_per_workgroup"], "pool_bytes": b.info()["matrix_bytes"], "fill_us": round(us, 1)}), flush=True)
        return [x.copy() for x in b.results()]

    # (short reads: queries 100 - 130 under references 100 - 160, so that |m - n| < 64 and BANW admits every pair)
    work = [(f"{args.pairs} x 4096^2 related", lambda prefix: related(args.pairs, 4096, 43, prefix=prefix), args.band, True, True),
            (f"{args.short_reads} short reads", lambda prefix: make_ragged_batch(args.short_reads, 100, 130, 100, 160, seed=44), 64, True, False)]
    if args.long_pairs:
        work.append((f"{args.long_pairs} x 30000^2", lambda prefix: related(args.long_pairs, 30000, 47, gap=150, prefix=prefix), 256, False, True))
    for name, gen, band, int16_admits, has_prefix in work:
        made = {}
        for mode, algo, with_table, z, prefix in MODES:
            if prefix and not has_prefix:
                continue
            key = 1024 if prefix else 0
            if key not in made:
                made[key] = gen(key)
            sb = made[key]
            sides = ["DIR"] if args.dir_only else ["DIR", "LONG"] + (["INT16"] if int16_admits and not (with_table and algo in ("BSW", "BASW")) else [])
            batches = {side: make(side, algo, sb, band, with_table, z) for side in sides}
            try:
                seen = {}
                for rep in range(args.reps):
                    for side in (sides if rep % 2 == 0 else sides[::-1]):
                        got = measure(batches[side], name, mode, side, band)
                        seen.setdefault(side, got)
                        for x, y in zip(got, seen["DIR"] if "DIR" in seen else got):  # every side, every repetition: the same results
                            assert np.array_equal(x, y), (name, mode, side, rep)
                assert set(seen) == set(sides)
                if "LONG" in batches:
                    d = batches["LONG"].describe()
                    assert d["kernel"] in ("k_bscore_fill", "k_lscore_fill") and d["store"] == 0 and batches["LONG"].info()["matrix_bytes"] == 0, d
            finally:
                for b in batches.values():
                    b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--fills", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--band", type=int, default=128)
    ap.add_argument("--short-reads", type=int, default=100000)
    ap.add_argument("--long-pairs", type=int, default=256)
    ap.add_argument("--dir-only", action="store_true", help="time the direction fills alone (a build without the flag)")
    ap.add_argument("--package", default=ROOT, help="directory that holds the dpx_gpu_genomics_project_amd package to measure")
    ap.add_argument("--child-timeout", type=float, default=400.0, help="seconds after which a child process is killed")
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
            recs.append(rec)
        print(f"process {proc}: {sum(r['process'] == proc for r in recs)} measurements", flush=True)
    print(f"summary, package {os.path.relpath(os.path.abspath(args.package), ROOT)}, weights {W}: fill time, median [min, max] over {args.processes} fresh "
          f"processes of each process's median ({args.reps} measurements of {args.fills} fills); all sides gave equal results in every child")
    for name, mode in dict.fromkeys((r["workload"], r["mode"]) for r in recs):
        base = None
        for side in SIDES:
            mine = [r for r in recs if (r["workload"], r["mode"], r["side"]) == (name, mode, side)]
            per = [statistics.median([r["fill_us"] for r in mine if r["process"] == p]) for p in range(args.processes) if any(r["process"] == p for r in mine)]
            if not per:
                continue
            med = statistics.median(per)
            base = med if side == "DIR" else base
            print(f"  {name:28s} {mode:30s} {side:5s} {mine[0]['kernel']:14s} band {mine[0]['band']:3d} C {mine[0]['cells_per_lane']} wpb {mine[0]['waves_per_workgroup']} "
                  f"pool {mine[0]['pool_bytes'] / 1e9:6.3f} GB {med / 1e3:9.3f} ms [{min(per) / 1e3:.3f}, {max(per) / 1e3:.3f}]"
                  + (f"  x{med / base:.3f} of the direction fill" if base and side != "DIR" else ""))


if __name__ == "__main__":
    main()
