#!/usr/bin/env python3
"""A/B of a DPX_KEEP_BAND_DIRECTIONS batch against the DPX_KEEP_MATRICES batch of the same seeded pairs, for BANW and BAXT, every
measurement in a FRESH process (its own pool), the two kinds of process alternating:

  * the fill of --pairs pairs of --m x --n at --band (the README's banded shape: 10 000 x 4096^2, band 128), with the bytes each batch
    writes and the fraction of the 8 TB/s HBM roofline from its algorithmic bytes;
  * the output (traceback + text kernels, dpx_batch_last_output_usec) of --tb-pairs of them;
  * one long-read shape that only the direction batch admits (--long-pairs pairs of --long-m x --long-n at the usual mapper weights
    2 / -4 / -4 / -2: the matrix batch is DPX_ERR_RANGE, which the tool checks).

A process runs one discarded warm-up fill, then one timed pass of --fills back-to-back fills (dpx_batch_fill_timed); its figure is the
mean of those fills.  --passes processes per case; the report gives their median, minimum and maximum.  One JSON line per process, then
a summary.  No ratio is promised: the tool measures.  Needs a GPU.

--ab OLD.so NEW.so compares two builds of the library instead (DPX_LIB), by the method and rule of profiles/band_sharing_ab.md: direction
batches only, 4096 x 4096 pairs, weights 2 / -3 / -5 / -1, --passes fresh processes per library and case, strictly alternating; the new
median must be at most the old median plus the old max - min.  Cases: the fills of BANW and BAXT at bands 64, 128, 256 and 512 (600
pairs, 512 at band 512), then traceback + text of --tb-pairs pairs at band 128 for BANW and BAXT, one-piece and two-piece (DPX_TWO_PIECE_GAPS:
weights 2 / -4 / -4 / -2 and a second piece -24 / -1).  --ab-only fills | walks runs one half."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W = (3, -1, -3, -1)
AB_W = (2, -3, -5, -1)
TWO_W, TWO_SECOND = (2, -4, -4, -2), (-24, -1)
MAPPER = (2, -4, -4, -2)
HBM_BYTES_PER_S = 8e12
ALGOS = {"BANW": 7, "BAXT": 10}


def child(args):
    import dpx_gpu_genomics_project_amd as dpx
    from dpx_gpu_genomics_project_amd.synth import make_batch

    dpx.init(0)
    sb = make_batch(args.pairs, args.m, args.n, seed=args.seed)
    w = MAPPER if args.mapper else TWO_W if args.two_piece else AB_W if args.ab_weights else W
    keep = dpx.KEEP_BAND_DIRECTIONS if args.kind == "directions" else dpx.KEEP_MATRICES
    if args.two_piece:
        keep |= dpx.TWO_PIECE_GAPS
    rec = {"algo": args.child, "kind": args.kind, "pairs": args.pairs, "m": args.m, "n": args.n, "band": args.band, "weights": w}
    try:
        b = dpx.Batch(ALGOS[args.child], sb.sequences, sb.pairs, *w, band=args.band, flags=keep | dpx.TIME_FILLS)
    except dpx.DpxError as e:
        rec["status"] = e.status
        print(json.dumps(rec), flush=True)
        return
    with b:
        if args.two_piece:
            b.set_second_gap(*TWO_SECOND)
        b.fill_timed(1)  # warm-up (first touch of the pool, code load): discarded
        us = b.fill_timed(args.fills)
        info, d = b.info(), b.describe()
        rec.update(status=0, kernel=d["kernel"], cells_per_lane=d["rows_per_lane"], fill_us=round(us, 1), algorithmic_bytes=info["algorithmic_bytes"],
                   matrix_bytes=info["matrix_bytes"], roofline_fraction=round(info["algorithmic_bytes"] / (us * 1e-6) / HBM_BYTES_PER_S, 3))
        if args.tb:
            out = C.c_double(0.0)
            times = []
            for _ in range(args.fills):  # a fill invalidates the lines: every output_begin walks again
                b.fill()
                b.output_begin(0)
                b.output_end()
                assert dpx.load().dpx_batch_last_output_usec(b._h, C.byref(out)) == 0
                times.append(out.value)
            rec.update(traceback=d.get("traceback", ""), output_us=round(statistics.median(times), 1))
    print(json.dumps(rec), flush=True)


def run(algo, kind, pairs, m, n, args, tb=False, mapper=False, lib=None, band=None, extra=()):
    env = dict(os.environ)
    env.pop("DPX_TB_WALK", None)
    if lib:
        env["DPX_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", algo, "--kind", kind, "--pairs", str(pairs), "--band", str(band or args.band), "--m", str(m),
           "--n", str(n), "--fills", str(args.fills), "--seed", str(args.seed)] + (["--tb"] if tb else []) + (["--mapper"] if mapper else []) + list(extra)
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.timeout)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} failed ({r.returncode}): {r.stderr[-800:]!r}")
    rec = json.loads(r.stdout.decode().strip().splitlines()[-1])
    print(json.dumps(rec), flush=True)
    return rec


def spread(recs, key="fill_us"):
    v = [r[key] for r in recs]
    return statistics.median(v), min(v), max(v)


def fmt(t):
    md, lo, hi = t
    return f"{md / 1e3:9.3f} ms [{lo / 1e3:.3f} .. {hi / 1e3:.3f}]"


def ab(args):
    """two builds of the library, direction batches only; a table in the format of profiles/band_sharing_ab.md"""
    old_lib, new_lib = args.ab
    cases = []
    if args.ab_only in ("", "fills"):
        cases += [(f"{algo} fill, `k_bdir_fill<EXT = {'true' if algo == 'BAXT' else 'false'}>`, band {band}", algo, 512 if band == 512 else 600, band, False, ["--ab-weights"], "fill_us")
                  for algo in ("BANW", "BAXT") for band in (64, 128, 256, 512)]
    if args.ab_only in ("", "walks"):
        cases += [(f"{algo} traceback + text, {'two-piece' if two else 'one-piece'}, band 128", algo, args.tb_pairs, 128, True, ["--two-piece"] if two else ["--ab-weights"], "output_us")
                  for two in (False, True) for algo in ("BANW", "BAXT")]
    rows = []
    for name, algo, pairs, band, tb, extra, key in cases:
        got = {old_lib: [], new_lib: []}
        for _ in range(args.passes):  # strictly alternating fresh processes
            for lib in (old_lib, new_lib):
                got[lib].append(run(algo, "directions", pairs, args.m, args.n, args, tb=tb, lib=lib, band=band, extra=extra)[key])
        (om, olo, ohi), nm = (statistics.median(got[old_lib]), min(got[old_lib]), max(got[old_lib])), statistics.median(got[new_lib])
        rows.append(f"| {name} | {pairs} | {om:.1f} | {ohi - olo:.1f} | {nm:.1f} | {(nm / om - 1) * 100:+.1f} % | {'met' if nm <= om + (ohi - olo) else 'MISSED'} |"
                    f"{' (old spread above 3 % of its median)' if ohi - olo > 0.03 * om else ''}")
        print(rows[-1], flush=True)
    print("| case | pairs | before: median us | before: max - min us | after: median us | change | rule |\n|---|---|---|---|---|---|---|")
    print("\n".join(rows))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--kind", default="directions", choices=["directions", "matrices"])
    ap.add_argument("--tb", action="store_true")
    ap.add_argument("--mapper", action="store_true")
    ap.add_argument("--pairs", type=int, default=10000)
    ap.add_argument("--band", type=int, default=128)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--fills", type=int, default=5)
    ap.add_argument("--passes", type=int, default=5, help="fresh processes per case")
    ap.add_argument("--seed", type=int, default=43)
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--algos", default="BANW,BAXT")
    ap.add_argument("--tb-pairs", type=int, default=1712)
    ap.add_argument("--long-pairs", type=int, default=2000)
    ap.add_argument("--long-m", type=int, default=20000)
    ap.add_argument("--long-n", type=int, default=20000)
    ap.add_argument("--two-piece", action="store_true", help="child: a DPX_TWO_PIECE_GAPS batch")
    ap.add_argument("--ab-weights", action="store_true", help="child: weights 2 / -3 / -5 / -1")
    ap.add_argument("--ab", nargs=2, metavar=("OLD.so", "NEW.so"), default=None)
    ap.add_argument("--ab-only", default="", choices=["", "fills", "walks"])
    args = ap.parse_args()
    if args.child:
        return child(args)
    if args.ab:
        return ab(args)
    lines = []
    for algo in [a for a in args.algos.split(",") if a]:
        got = {"directions": [], "matrices": []}
        for _ in range(args.passes):  # alternating fresh processes
            for kind in got:
                got[kind].append(run(algo, kind, args.pairs, args.m, args.n, args))
        d0, m0 = got["directions"][0], got["matrices"][0]
        lines.append(f"  {algo} fill, {args.pairs} x {args.m}x{args.n} band {args.band}: directions {fmt(spread(got['directions']))} ({d0['matrix_bytes'] / 2**30:.2f} GiB, roofline "
                     f"{d0['algorithmic_bytes'] / (spread(got['directions'])[0] * 1e-6) / HBM_BYTES_PER_S:.3f})   matrices {fmt(spread(got['matrices']))} "
                     f"({m0['matrix_bytes'] / 2**30:.2f} GiB, roofline {m0['algorithmic_bytes'] / (spread(got['matrices'])[0] * 1e-6) / HBM_BYTES_PER_S:.3f})")
        tb = {"directions": [], "matrices": []}
        for _ in range(args.passes):
            for kind in tb:
                tb[kind].append(run(algo, kind, args.tb_pairs, args.m, args.n, args, tb=True))
        lines.append(f"  {algo} traceback + text, {args.tb_pairs} pairs: directions ({tb['directions'][0]['traceback']}) {fmt(spread(tb['directions'], 'output_us'))}   "
                     f"matrices ({tb['matrices'][0]['traceback']}) {fmt(spread(tb['matrices'], 'output_us'))}")
        refused = run(algo, "matrices", args.long_pairs, args.long_m, args.long_n, args, mapper=True)
        assert refused["status"] == -4, refused  # DPX_ERR_RANGE: the int16 planes cannot hold this shape
        long = [run(algo, "directions", args.long_pairs, args.long_m, args.long_n, args, tb=True, mapper=True) for _ in range(args.passes)]
        lines.append(f"  {algo} long reads, {args.long_pairs} x {args.long_m}x{args.long_n} band {args.band}, weights {MAPPER} (matrix batch: DPX_ERR_RANGE): fill "
                     f"{fmt(spread(long))} ({long[0]['matrix_bytes'] / 2**30:.2f} GiB)   traceback + text {fmt(spread(long, 'output_us'))}")
    print("summary: median over the processes [min .. max]")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
