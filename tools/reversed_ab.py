#!/usr/bin/env python3
"""A/B of per-pair orientation (dpx_batch_set_reversed) against what a caller did before it, after tools/bdx_ab.py's method: the same
seeded pairs in every process, one fresh child process per repetition (the parent never opens the GPU), median [min, max] over the
children.  Workloads: --short-reads short reads on a BAXT matrix batch at band 64, every pair reversed; --pairs x 4096^2 at band 128
on a band-direction batch, every second pair reversed; --long-pairs x 30 000^2 at band 256 on a band-direction batch, every second
pair reversed.  Per workload and child, each --reps times:

  fill U1, U2   dpx_batch_fill_timed of two unmasked batches of the same pairs: the spread two equal batches show
  fill M        the same on the masked batch (the same kernels and plan, strings at other addresses)
  fill M off    the same batch and pool again with the mask cleared: against fill M it shows the mask alone, without the difference
                between two pools; `fill M again` / `fill M off again`: both once more in the same order, which shows what the order
                of two measurements is worth
  setter        (a) dpx_batch_set_reversed until the batch's stream is idle (wall): the copies of the flagged strings on the device;
                `setter again`: the same call once more on the same batch, whose allocation is then a recycled one
  out U / out M (b) dpx_batch_fill + dpx_batch_cigars_begin / _end (wall) without and with the mask: the difference is the flip of the
                lines and the mapping of the records
  before        (c) the caller's way before the setter: the flagged strings reversed on the host with numpy (`host_reverse`), a plain
                batch created from that buffer, upload included (`create`, against `create U` for the original buffer), the same fill
                and CIGARs, and the ops and coordinates of the flagged pairs turned round on the host with numpy (`host_flip`)

(c) depends on the host and on numpy: the bytes reversed and the ops flipped are printed so that it can be scaled.  Needs a GPU.  A
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

W = (2, -3, -5, -1)


def related(count, size, seed):
    """`count` pairs of `size` bases, the query the reference with 8 % substitutions"""
    from dpx_gpu_genomics_project_amd.synth import from_strings

    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    texts = []
    for _ in range(count):
        ref = rng.integers(0, 4, size)
        q = ref.copy()
        sub = rng.random(size) < 0.08
        q[sub] = rng.integers(0, 4, int(sub.sum()))
        texts.append((acgt[ref].tobytes(), acgt[q].tobytes()))
    return from_strings(texts)


def _spans(starts, lens):
    """for strings at `starts` of `lens` bytes: (position of every byte, position of the byte that is its mirror image)"""
    total = int(lens.sum())
    begin = np.cumsum(lens) - lens
    pos = np.arange(total, dtype=np.int64) - np.repeat(begin, lens)
    return np.repeat(starts, lens) + pos, np.repeat(starts + lens - 1, lens) - pos


def host_reverse(seq, pairs, mask):
    """the buffer with both strings of every flagged pair reversed where they stand (the pairs of these workloads share no bytes)"""
    k = np.flatnonzero(mask)
    starts = np.concatenate([pairs["referenceIdx"][k], pairs["queryIdx"][k]]).astype(np.int64)
    lens = np.concatenate([pairs["referenceSize"][k], pairs["querySize"][k]]).astype(np.int64)
    dst, src = _spans(starts, lens)
    out = seq.copy()
    out[dst] = seq[src]
    return out, int(lens.sum())


def host_flip(records, ops, pairs, mask):
    """ops of the flagged pairs in reverse order, their coordinates counted from the other end"""
    k = np.flatnonzero(mask)
    dst, src = _spans(records["opsOffset"][k].astype(np.int64), records["numOps"][k].astype(np.int64))
    out = ops.copy()
    out[dst] = ops[src]
    rec = records.copy()
    n, m = pairs["referenceSize"][k], pairs["querySize"][k]
    rec["refStart"][k], rec["refEnd"][k] = n - records["refEnd"][k], n - records["refStart"][k]
    rec["qryStart"][k], rec["qryEnd"][k] = m - records["qryEnd"][k], m - records["qryStart"][k]
    return rec, out


def child(args):
    import dpx_gpu_genomics_project_amd as dpx
    from dpx_gpu_genomics_project_amd.synth import make_ragged_batch

    dpx.init(0)
    work = []
    if args.short_reads:
        work.append((f"{args.short_reads} short reads", make_ragged_batch(args.short_reads, 80, 130, 100, 160, seed=44), 64, dpx.KEEP_MATRICES, 1))
    if args.pairs:
        work.append((f"{args.pairs} x 4096^2", related(args.pairs, 4096, 43), 128, dpx.KEEP_BAND_DIRECTIONS, 2))
    if args.long_pairs:
        work.append((f"{args.long_pairs} x 30000^2", related(args.long_pairs, 30000, 47), 256, dpx.KEEP_BAND_DIRECTIONS, 2))

    def ms(t0):
        return round((time.perf_counter() - t0) * 1e3, 3)

    def outputs(b):
        t0 = time.perf_counter()
        b.fill()
        b.cigars_begin()
        recs, ops = b.cigars_end()
        return ms(t0), recs, ops

    for name, sb, band, flags, every in work:
        mask = (np.arange(sb.num_pairs) % every == 0).astype(np.uint8)

        def batch(seq):
            return dpx.Batch(dpx.ALGO_BAXT, seq, sb.pairs, *W, band=band, flags=flags)

        for rep in range(args.reps):
            rec = {"workload": name, "band": band, "masked": int(mask.sum()), "pairs": sb.num_pairs}
            with batch(sb.sequences) as u1, batch(sb.sequences) as u2:
                for b in (u1, u2):
                    b.fill_timed(1)   # warm-up (first touch of the pool, code load): discarded
                rec["fill U1"], rec["fill U2"] = round(u1.fill_timed(args.fills) / 1e3, 3), round(u2.fill_timed(args.fills) / 1e3, 3)
                outputs(u1)           # (its buffers exist from here on)
                rec["out U"], urec, uops = outputs(u1)
                rec["kernel"] = u1.describe()["kernel"]
            t0 = time.perf_counter()
            with batch(sb.sequences) as m:
                rec["create U"] = ms(t0)
                m.sync()
                t0 = time.perf_counter()
                m.set_reversed(mask)
                m.sync()
                rec["setter"] = ms(t0)
                m.fill_timed(1)
                rec["fill M"] = round(m.fill_timed(args.fills) / 1e3, 3)
                m.set_reversed(None)
                m.fill_timed(1)
                rec["fill M off"] = round(m.fill_timed(args.fills) / 1e3, 3)
                t0 = time.perf_counter()
                m.set_reversed(mask)
                m.sync()
                rec["setter again"] = ms(t0)   # (the allocation is a parked one this time)
                m.fill_timed(1)
                rec["fill M again"] = round(m.fill_timed(args.fills) / 1e3, 3)
                m.set_reversed(None)
                m.fill_timed(1)
                rec["fill M off again"] = round(m.fill_timed(args.fills) / 1e3, 3)
                m.set_reversed(mask)
                outputs(m)
                rec["out M"], mrec, mops = outputs(m)
                rec["rev_bytes"] = m.describe()["rev_bytes"]
            t0 = time.perf_counter()
            turned, nbytes = host_reverse(sb.sequences, sb.pairs, mask)
            rec["host_reverse"], rec["bytes_reversed"] = ms(t0), nbytes
            t0 = time.perf_counter()
            with batch(turned) as c:
                rec["create"] = ms(t0)
                outputs(c)
                rec["out before"], crec, cops = outputs(c)
                t0 = time.perf_counter()
                frec, fops = host_flip(crec, cops, sb.pairs, mask)
                rec["host_flip"], rec["ops"] = ms(t0), int(len(cops))
            rec["same"] = bool(frec.tobytes() == mrec.tobytes() and np.array_equal(fops, mops))   # both ways report the same alignments
            print(json.dumps(rec), flush=True)


FIELDS = ("fill U1", "fill U2", "fill M", "fill M off", "fill M again", "fill M off again", "setter", "setter again", "out U", "out M", "create U", "host_reverse", "create", "out before", "host_flip")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fills", type=int, default=5)
    ap.add_argument("--short-reads", type=int, default=100000)
    ap.add_argument("--pairs", type=int, default=10000)
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
    print(f"summary in ms: median [min, max] over {args.processes} fresh processes of each process's median ({args.reps} measurements; fills: "
          f"{args.fills} timed fills each)")
    for name in dict.fromkeys(r["workload"] for r in recs):
        mine = [r for r in recs if r["workload"] == name]
        first = mine[0]
        print(f"  {name}: band {first['band']}, {first['kernel']}, {first['masked']} of {first['pairs']} pairs reversed, {first['bytes_reversed']} bytes "
              f"of strings reversed, {first['ops']} ops, allocation of the setter {first['rev_bytes']} bytes, both ways agree: {all(r['same'] for r in mine)}")
        med = {}
        for f in FIELDS:
            per = [statistics.median([r[f] for r in mine if r["process"] == p]) for p in range(args.processes)]
            med[f] = statistics.median(per)
            print(f"    {f:14s} {med[f]:10.3f} [{min(per):.3f}, {max(per):.3f}]")
        print(f"    fill M / fill U1 = {med['fill M'] / med['fill U1']:.4f}, fill U2 / fill U1 = {med['fill U2'] / med['fill U1']:.4f}, "
              f"fill M / fill M off = {med['fill M'] / med['fill M off']:.4f}, again {med['fill M again'] / med['fill M off again']:.4f}")
        print(f"    device side: setter + (out M - out U) = {med['setter'] + med['out M'] - med['out U']:.3f}; host side before: host_reverse + "
              f"host_flip = {med['host_reverse'] + med['host_flip']:.3f}")


if __name__ == "__main__":
    main()
