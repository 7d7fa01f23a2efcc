#!/usr/bin/env python3
"""A/B of DPX_ALGO_BASW (banded affine-gap Smith-Waterman): mean fill time over dpx_batch_fill_timed, every measurement in a FRESH process
(its own matrix pool), on the same seeded pairs of 4096 x 4096:

  * BASW at band 128 (and 64 / 256 / 512 beside it; wider bands run fewer pairs, so that three planes stay under --pool-gb), with its fraction of the 8 TB/s HBM roofline from the batch's algorithmic bytes;
  * BSW at the same bands (one plane: a third of the bytes);
  * unbanded ASW on the first --asw-pairs pairs (three full planes: 256 pairs are about 26 GB), with the library given by --asw-lib
    (a build of the commit before BASW, to compare against; default: the in-tree library);
  * with --controls: ASW / BSW / ANW control workloads on both libraries, to show that the existing kernels' times did not move.

Every process runs one discarded warm-up fill, then --passes passes of --fills back-to-back fills; a pass's figure is the mean of its
fills, the report gives the mean over the passes and their spread (min .. max).  One JSON line per process, then a summary.  Needs a GPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = (3, -1, -3, -1)
HBM_BYTES_PER_S = 8e12


def child(args):
    import dpx_gpu_genomics_project_amd as dpx
    from dpx_gpu_genomics_project_amd.synth import make_batch

    dpx.init(0)
    algo = {"BASW": 5, "ASW": dpx.ALGO_ASW, "BSW": dpx.ALGO_BSW, "ANW": dpx.ALGO_ANW}[args.child]
    sb = make_batch(args.pairs, args.m, args.n, seed=args.seed)
    w = (3, -1, -2, -1) if args.child == "BSW" else W
    with dpx.Batch(algo, sb.sequences, sb.pairs, *w, band=args.band, flags=dpx.KEEP_MATRICES | dpx.TIME_FILLS) as b:
        b.fill_timed(1)  # warm-up (first touch of the pool, code load): discarded
        passes = [b.fill_timed(args.fills) for _ in range(args.passes)]
        info, d = b.info(), b.describe()
    mean = statistics.mean(passes)
    print(json.dumps({"algo": args.child, "lib": os.environ.get("DPX_LIB", "in-tree"), "pairs": args.pairs, "m": args.m, "n": args.n, "band": args.band,
                      "kernel": d["kernel"], "cells_per_lane": d["rows_per_lane"], "fill_us_mean": round(mean, 1), "fill_us_min": round(min(passes), 1),
                      "fill_us_max": round(max(passes), 1), "passes": [round(p, 1) for p in passes], "algorithmic_bytes": info["algorithmic_bytes"],
                      "matrix_bytes": info["matrix_bytes"], "roofline_fraction": round(info["algorithmic_bytes"] / (mean * 1e-6) / HBM_BYTES_PER_S, 3)}),
          flush=True)


def run(algo, pairs, band, args, lib=None, m=4096, n=4096):
    env = dict(os.environ)
    env.pop("DPX_LIB", None)
    if lib:
        env["DPX_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", algo, "--pairs", str(pairs), "--band", str(band), "--m", str(m), "--n", str(n),
           "--fills", str(args.fills), "--passes", str(args.passes), "--seed", str(args.seed)]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.timeout)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed ({r.returncode}): {r.stderr[-800:]!r}")
    rec = json.loads(r.stdout.decode().strip().splitlines()[-1])
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--asw-pairs", type=int, default=256)
    ap.add_argument("--asw-lib", default=None, help="library of the commit before BASW (for the unbanded ASW fill and the controls)")
    ap.add_argument("--band", type=int, default=128)
    ap.add_argument("--bands", default="128,64,256,512")
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--fills", type=int, default=5)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--seed", type=int, default=43)
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--pool-gb", type=float, default=64.0, help="cap on a BASW batch's matrix bytes: wider bands run fewer pairs (BSW the same number)")
    ap.add_argument("--controls", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    recs = []
    bands = [int(x) for x in args.bands.split(",")]
    count = {}
    for band in bands:
        cpl = 1 if band <= 64 else 2 if band <= 128 else 4 if band <= 256 else 8  # dpx_layout.h: cells per lane, 16 / (2 * cpl) steps per 1-KiB chunk
        per_pair = 3 * 1024 * -(-(args.m + args.n - 1) // max(1, 8 // cpl))
        count[band] = max(64, min(args.pairs, int(args.pool_gb * 2**30 / per_pair)))
        recs.append(run("BASW", count[band], band, args))
        recs.append(run("BSW", count[band], band, args))
    # the same pairs (same seed: the first --asw-pairs of them) on both sides of the banded / unbanded comparison
    recs.append(run("BASW", args.asw_pairs, bands[0], args))
    recs.append(run("ASW", args.asw_pairs, 0, args, lib=args.asw_lib))
    if args.controls:
        for lib in (args.asw_lib, None):
            recs.append(run("ASW", 1000, 0, args, lib=lib, m=1024, n=1024))
            recs.append(run("ANW", 1000, 0, args, lib=lib, m=1024, n=1024))
            recs.append(run("BSW", args.pairs, 128, args, lib=lib))
    print("summary: mean fill time over the passes [min .. max], ms")
    for r in recs:
        print(f"  {r['algo']:4s} {r['pairs']:6d} x {r['m']}x{r['n']} band {r['band']:3d} {r['kernel']:16s} lib={os.path.basename(r['lib']):24s} "
              f"{r['fill_us_mean'] / 1e3:9.3f} [{r['fill_us_min'] / 1e3:.3f} .. {r['fill_us_max'] / 1e3:.3f}]  alg {r['algorithmic_bytes'] / 1e9:7.2f} GB  "
              f"roofline {r['roofline_fraction']:.3f}")
    by = {(r["algo"], r["pairs"], r["band"], r["lib"] == "in-tree" or r["algo"] != "ASW"): r for r in recs}
    for band in bands:
        a, l = by.get(("BASW", count[band], band, True)), by.get(("BSW", count[band], band, True))
        if a and l:
            print(f"  band {band}: BASW / BSW = {a['fill_us_mean'] / l['fill_us_mean']:.2f} (bytes: 3.00)")
    small = [r for r in recs if r["pairs"] == args.asw_pairs and r["m"] == args.m]
    if len(small) >= 2:
        print(f"  {args.asw_pairs} pairs: unbanded ASW / BASW band {bands[0]} = {small[1]['fill_us_mean'] / small[0]['fill_us_mean']:.1f}")


if __name__ == "__main__":
    main()
