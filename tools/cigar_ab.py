#!/usr/bin/env python3
"""A/B of the two output paths of a filled batch, in one process: the text pipeline (dpx_batch_output_begin + _end: three lines per
pair, formatted on the device) against the CIGAR path (dpx_batch_cigars_begin + _end: one 48-byte record per pair and the packed ops).
One batch per workload; the two paths alternate --reps times (at least seven) after one warm-up of each, the order reversed every other
rep; the batch is refilled and synchronised in front of every measurement, so the traceback lines are invalid and both paths pay the
walk; each path is timed with the host clock around its pair of calls (_end returns after a stream synchronise).  Workloads:
100 000 short reads under LSW, 1000 x 1024^2 under ANW, 4000 x 4096^2 at band 128 under BAXT.  Prints one JSON line per measurement
with the bytes the path copied to the host, then a summary (median [min, max]) per workload.  The text path is the yardstick.
Needs a GPU."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dpx_gpu_genomics_project_amd as dpx  # noqa: E402
from dpx_gpu_genomics_project_amd.synth import make_batch, make_ragged_batch  # noqa: E402


def text_path(b):
    """straight through the C ABI: the wrappers of capi.py copy the results once more on the host, which is not what is measured"""
    text, nbytes, offs = C.c_char_p(), C.c_size_t(0), C.POINTER(C.c_uint64)()
    t0 = time.perf_counter()
    rc = b._lib.dpx_batch_output_begin(b._h, 0) or b._lib.dpx_batch_output_end(b._h, C.byref(text), C.byref(nbytes), C.byref(offs))
    dt = time.perf_counter() - t0
    assert rc == 0, rc
    # what the two calls copy: numPairs + 1 offsets, numPairs alignment lengths, the text
    return dt, nbytes.value + 8 * (b.num_pairs + 1) + 4 * b.num_pairs


def cigar_path(b):
    recs, ops, n = C.c_void_p(), C.c_void_p(), C.c_uint64(0)
    t0 = time.perf_counter()
    rc = b._lib.dpx_batch_cigars_begin(b._h, dpx.CIGAR_EXTENDED) or b._lib.dpx_batch_cigars_end(b._h, C.byref(recs), C.byref(ops), C.byref(n))
    dt = time.perf_counter() - t0
    assert rc == 0, rc
    # what the two calls copy: the records with the total behind them, the ops
    return dt, dpx.ALIGNMENT_DTYPE.itemsize * b.num_pairs + 8 + 4 * n.value


PATHS = {"text": text_path, "cigar": cigar_path}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--short-reads", type=int, default=100000)
    ap.add_argument("--mid-pairs", type=int, default=1000)
    ap.add_argument("--long-pairs", type=int, default=4000)
    ap.add_argument("--band", type=int, default=128)
    args = ap.parse_args()
    assert args.reps >= 7, "at least seven alternations"
    dpx.init(0)
    work = [(f"{args.short_reads} short reads", "LSW", dpx.ALGO_LSW, (3, -1, -2, -1), 0, lambda: make_ragged_batch(args.short_reads, 80, 130, 100, 160, seed=44)),
            (f"{args.mid_pairs} x 1024^2", "ANW", dpx.ALGO_ANW, (3, -1, -3, -1), 0, lambda: make_batch(args.mid_pairs, 1024, 1024, seed=45)),
            (f"{args.long_pairs} x 4096^2, band {args.band}", "BAXT", dpx.ALGO_BAXT, (3, -1, -3, -1), args.band, lambda: make_batch(args.long_pairs, 4096, 4096, seed=43))]
    recs = []
    for name, algo, code, w, band, make in work:
        sb = make()
        with dpx.Batch(code, sb.sequences, sb.pairs, *w, band=band) as b:
            def measure(path, keep):
                b.fill()
                b.sync()  # (the refill invalidates the traceback lines: the path measured next pays the walk)
                dt, nbytes = PATHS[path](b)
                if keep:
                    recs.append({"workload": name, "algo": algo, "path": path, "ms": round(dt * 1e3, 3), "d2h_bytes": int(nbytes)})
                    print(json.dumps(recs[-1]), flush=True)
            for path in PATHS:
                measure(path, keep=False)  # warm-up: buffers, code load
            for rep in range(args.reps):
                for path in (list(PATHS) if rep % 2 == 0 else list(PATHS)[::-1]):
                    measure(path, keep=True)
    print(f"summary: host time of begin + end, median [min, max] over {args.reps} alternations; D2H bytes of one run")
    for name, algo, *_ in work:
        stat = {}
        for path in PATHS:
            rs = [r for r in recs if r["workload"] == name and r["path"] == path]
            v = [r["ms"] for r in rs]
            stat[path] = (statistics.median(v), min(v), max(v), rs[0]["d2h_bytes"])
            print(f"  {name:34s} {algo:4s} {path:5s} {stat[path][0]:9.3f} ms [{stat[path][1]:.3f}, {stat[path][2]:.3f}]  D2H {stat[path][3]:>12d} B")
        print(f"  {name:34s} {algo:4s} cigar / text: time {stat['cigar'][0] / stat['text'][0]:.2f}, bytes {stat['cigar'][3] / stat['text'][3]:.3f}")


if __name__ == "__main__":
    main()
