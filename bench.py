#!/usr/bin/env python3
"""bench.py -- headline benchmark of the MI355X pairwise-alignment DP engine.

Metric (BASELINE.json): GCUPS = sum(refLen*queryLen) / seconds / 1e9 (the reference's own formula,
cuda/LNW/LinearNeedlemanWunschV12.cu:487-491) on a 10k-pair 1024x1024 LinearSmithWaterman batch PER GPU
(weak scaling: every rank owns an independent 10k-pair sub-batch; the only collective is one RCCL gather of
the int32 scores to rank 0 per step).  A "step" = one DP fill of the whole resident batch, int16 score matrix
written to HBM, + that gather.  Inputs are resident in HBM before the timed region.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]            # N=1
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ...

Prints ONE JSON line on rank 0: metric / value / unit / higher_is_better / dtype / ms_per_step (wall time of the K
timed steps / K) and the workload's config.  A plain run does only what that headline needs; --full adds
  "roofline":     algorithmic HBM bytes per fill / mean fill-kernel time (HIP events around every timed fill)
  "ranks":        every rank's fill-kernel ms, matrix-pool record and score checksum (rank 0 checks the gather)
  "cpu_baseline": the reference's own CPU classes (oracle/_ref, built by oracle/Makefile `make ref` where the
                  reference sources are present) or, if that binary is absent, the C oracle port -- timed on this
                  host's cores on a bounded sample of the same batch.  Reported beside the GPU number, never measured as it.
--dump-outputs DIR writes what the last timed step computed (rank 0) as DIR/<name>.npy: scores and end cells of every pair
(float64) and the score matrices of a seeded sample of pairs (float32).  Inputs are seeded, so equal arguments give equal inputs.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X spec, /opt/skills/guides/MI355X_MICROARCH.md "HBM3E peak BW"

WORKLOADS = {
    # name: (algo, pairs/GPU, m, n, match, mismatch, gapOpen, gapExtend, seed)
    "lsw_10k_1024": ("LSW", 10000, 1024, 1024, 3, -1, -2, -1, 1),
    "lsw_1k_512": ("LSW", 1000, 512, 512, 3, -1, -2, -1, 2),
    "anw_1k_1024": ("ANW", 1000, 1024, 1024, 3, -1, -3, -1, 3),
    "lnw_10k_1024": ("LNW", 10000, 1024, 1024, 3, -1, -2, -1, 7),
    "bsw_10k_4096_b128": ("BSW", 10000, 4096, 4096, 3, -1, -2, -1, 4),  # band 128 (BASELINE.json configs[3])
    # the reference's own dataset shape (configs[0]: short reads, reference 100-160, query 80-130); m = n = 0 -> ragged
    # BASELINE.json configs[4]: 100k pairs in total, sharded over the ranks (strong scaling; 12.5k pairs = 27.8 GB per GPU at N = 8)
    "lsw_100k_1024_sharded": ("LSW", -100000, 1024, 1024, 3, -1, -2, -1, 5),
    "lnw_100k_short": ("LNW", 100000, 0, 0, 3, -1, -2, -1, 6),
    "lsw_100k_short": ("LSW", 100000, 0, 0, 3, -1, -2, -1, 6),
    "anw_100k_short": ("ANW", 100000, 0, 0, 3, -1, -3, -1, 6),
}
BAND = 128
DUMP_PAIRS = 4  # --dump-outputs: score matrices of this many pairs (seeded choice)
DUMP_MAX_CELLS = 1_100_000  # a matrix with more cells (banded 4096 x 4096) is dumped as a seeded sample of this many cells
DUMP_MAX_BYTES = 64 << 20


def kernel_source_hash() -> str:
    """sha256 over the sources every device kernel is built from (changes exactly when a kernel may have changed)."""
    import hashlib
    h = hashlib.sha256()
    for name in ("dpx_kernels.hip", "dpx_kernels.h", "dpx_layout.h", "dpx_prims.hpp"):
        h.update(open(os.path.join(ROOT, "dpx_gpu_genomics_project_amd", "csrc", name), "rb").read())
    return h.hexdigest()


class _DevArray:
    """Zero-copy view of engine-owned device memory for torch (RCCL gather source)."""

    def __init__(self, ptr: int, n: int):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i4", "data": (ptr, False), "version": 2}


def pool_record(desc: dict) -> dict:
    """The matrix pool as dpx_batch_describe reports it: how it was allocated (chunked virtual range or one hipMalloc), the
    hipMemset time of every candidate allocation the engine timed and which one it kept -- so that a slow run explains itself."""
    if "pool" not in desc:
        return None
    ms = [float(x) for x in str(desc.get("pool_memset_ms", "")).split(",") if x and x != "untimed"]
    nbytes = int(desc.get("pool_bytes", 0))
    kept = int(desc.get("pool_kept", 0))
    fills = [float(x) for x in str(desc.get("pool_fill_ms", "")).split(",") if x and x != "unshopped"]
    kinds = [x for x in str(desc.get("pool_kinds", "")).split(",") if x]
    return {"mode": desc["pool"], "bytes": nbytes, "chunk_mb": int(desc.get("pool_chunk_mb", 0)), "candidates_memset_ms": ms,
            "candidates_fill_ms": fills, "candidates_kind": kinds, "kept": kept,
            "memset_tbps": round(nbytes / (ms[kept] * 1e-3) / 1e12, 3) if len(ms) > kept and ms[kept] > 0 else None}


def dump_outputs(out_dir, batch, algo_name, gathered=None):
    """What the last fill computed, as a caller receives it: score and end cell of every pair (dpx_batch_results) and the int16
    score matrices (dpx_batch_matrix; H, and I / D of the affine algorithm) of DUMP_PAIRS seeded pairs, every value exact in the
    float type it is stored in.  `gathered`: the score vector rank 0 received from the gather (N > 1)."""
    import numpy as np

    import dpx_gpu_genomics_project_amd as dpx

    scores, end_row, end_col = batch.results()
    arrays = {"scores": scores, "end_row": end_row, "end_col": end_col}
    if gathered is not None:
        arrays["gathered_scores"] = gathered
    arrays = {k: np.asarray(v, np.float64) for k, v in arrays.items()}
    pairs = np.sort(np.random.default_rng(0).choice(batch.num_pairs, min(DUMP_PAIRS, batch.num_pairs), replace=False))
    arrays["matrix_pairs"] = pairs.astype(np.float64)
    kinds = [("H", dpx.MAT_H)] + ([("I", dpx.MAT_I), ("D", dpx.MAT_D)] if algo_name == "ANW" else [])
    for p in pairs:
        for tag, which in kinds:
            mat = batch.matrix(int(p), which).astype(np.float32)
            if mat.size > DUMP_MAX_CELLS:  # flat indices of the sample, ascending, seeded by the pair
                mat = mat.ravel()[np.sort(np.random.default_rng(int(p)).choice(mat.size, DUMP_MAX_CELLS, replace=False))]
            arrays[f"matrix_{tag}_pair{p}"] = mat
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_MAX_BYTES, f"--dump-outputs: {total} bytes"
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), a)


def cpu_baseline(sb, algo_name, match, mismatch, gap_open, gap_extend, budget_pairs, shape):
    """Time the reference CPU path on a bounded sample (first `budget_pairs` pairs of this rank's batch)."""
    import numpy as np
    from dpx_gpu_genomics_project_amd.synth import SynthBatch, write_pairs_file

    cores = os.cpu_count() or 1
    if algo_name == "BSW":
        budget_pairs = min(budget_pairs, 64)  # the banded oracle walks 4096 rows x 255 cells per pair
    npairs = min(budget_pairs, sb.num_pairs)
    end = int(sb.pairs["queryIdx"][npairs - 1] + sb.pairs["querySize"][npairs - 1] + 1)
    sample = SynthBatch(sb.sequences[:end], sb.pairs[:npairs], sb.m, sb.n)  # exactly the pairs that are timed
    ref_o2 = os.path.join(ROOT, "oracle", "_ref", "ref_driver_O2")
    ref_o0 = os.path.join(ROOT, "oracle", "_ref", "ref_driver")
    desc = f"first {npairs} pairs of the rank-0 batch ({shape}), fill = init_matrix+score_matrix"
    if os.path.exists(ref_o2) and algo_name in ("LSW", "LNW", "ANW"):
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "sample.txt")
            write_pairs_file(sample, path)
            args = [algo_name, path, str(match), str(mismatch), str(gap_open), str(gap_extend)]
            o2 = json.loads(subprocess.run([ref_o2, "time"] + args + [str(npairs)], capture_output=True, text=True, check=True).stdout)
            out = {"value": round(o2["fill_gcups"], 4), "unit": "GCUPS", "cores": min(20, cores), "host_cores": cores, "kind": "reference",
                   "sample": desc + "; reference classes built -O2, 20 pthreads x 20 pairs per batch (c++/main.cpp:18-19)",
                   "threads": 20, "align_gcups_O2": round(o2["align_gcups"], 4)}
            # every host core: as many concurrent 20-thread reference processes as fit the host (SURVEY 8d "all host cores"), each
            # timing its own 400-pair slice (one full 20 x 20 batch of the reference driver) of the same batch at the same time
            procs = max(1, min(cores // 20, sb.num_pairs // 400, 16))
            if procs > 1:
                files = []
                for k in range(procs):
                    lo, hi = 400 * k, 400 * (k + 1)
                    base = int(sb.pairs["queryIdx"][lo - 1] + sb.pairs["querySize"][lo - 1] + 1) if lo else 0  # start of pair lo's record
                    end_k = int(sb.pairs["queryIdx"][hi - 1] + sb.pairs["querySize"][hi - 1] + 1)
                    prs = sb.pairs[lo:hi].copy()
                    prs["referenceIdx"] -= base
                    prs["queryIdx"] -= base
                    fk = os.path.join(td, f"slice{k}.txt")
                    write_pairs_file(SynthBatch(sb.sequences[base:end_k], prs, sb.m, sb.n), fk)
                    files.append(fk)
                t0 = time.perf_counter()
                ps = [subprocess.Popen([ref_o2, "time", algo_name, fk] + args[2:] + ["400"], stdout=subprocess.PIPE, text=True) for fk in files]
                outs = [json.loads(p_.communicate()[0]) for p_ in ps]
                wall = time.perf_counter() - t0
                # the processes run side by side: throughput = all their cells / the slowest one's fill time
                out["value_all_cores"] = round(sum(o["cells"] for o in outs) / max(o["fill_sec"] for o in outs) / 1e9, 4)
                out["all_cores"] = {"processes": procs, "threads": 20 * procs, "host_cores": cores, "pairs": 400 * procs,
                                    "wall_sec_incl_align": round(wall, 2)}
            if os.path.exists(ref_o0):  # the reference's own flags (c++/Makefile:2), on a tenth of the sample
                n0 = max(npairs // 10, 1)
                o0 = json.loads(subprocess.run([ref_o0, "time"] + args + [str(n0)], capture_output=True, text=True, check=True).stdout)
                out["fill_gcups_O0"] = round(o0["fill_gcups"], 4)
                out["align_gcups_O0"] = round(o0["align_gcups"], 4)
            return out
    # fallback baseline: the C oracle port (still only a baseline -- never the measured product)
    import ctypes as C
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "all"], check=True)
    lib = C.CDLL(os.path.join(ROOT, "oracle", "liboracle.so"))
    lib.orc_fill_batch_timed.restype = C.c_double
    lib.orc_fill_batch_timed.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_int] * 6 + [C.c_void_p]
    scores = np.zeros(npairs, np.int32)
    code = {"LNW": 0, "LSW": 1, "ANW": 2, "BSW": 3}[algo_name]
    pairs = np.ascontiguousarray(sample.pairs)
    sec = lib.orc_fill_batch_timed(code, sample.sequences.ctypes.data, pairs.ctypes.data, npairs, match, mismatch, gap_open,
                                   gap_extend, 128, cores, scores.ctypes.data)
    return {"value": round(sample.cells / sec / 1e9, 4), "unit": "GCUPS", "cores": cores, "kind": "port",
            "sample": desc + f"; C oracle (gcc -O2), {cores} pthreads", "threads": cores}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", default="lsw_10k_1024", choices=sorted(WORKLOADS))
    ap.add_argument("--pairs", type=int, default=0, help="override pairs per GPU (debug)")
    ap.add_argument("--total-pairs", type=int, default=0, help="override the total pair count of a sharded (strong-scaling) workload (debug)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-pairs", type=int, default=4000, help="pairs of the CPU-baseline sample")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl = RCCL over xGMI (default). gloo + --share-gpu rehearses the N>1 path on a 1-GPU box")
    ap.add_argument("--share-gpu", action="store_true", help="all ranks use cuda:0 (rehearsal only; RCCL refuses this)")
    ap.add_argument("--dump-scores", default="", help="tests: every rank saves its local scores to PREFIX.rank<r>.npy, rank 0 "
                    "the gathered vector to PREFIX.gathered.npy (after the timed region)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR", help="after the timed steps rank 0 writes what the last step "
                    "computed as DIR/<name>.npy (float64 / float32, at most 64 MB)")
    ap.add_argument("--full", action="store_true", help="also the roofline and per-rank figures (HIP events around every timed "
                    "fill), the result checks and the CPU baseline; a plain run measures the headline only")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            sys.exit("bench.py --gpus N>1 must be launched with torch.distributed.run (one rank per GPU)")
        args.gpus = world

    import numpy as np
    import torch
    import torch.distributed as dist

    import dpx_gpu_genomics_project_amd as dpx

    if not torch.cuda.is_available():
        sys.exit("bench.py needs a GPU: the engine has no CPU fallback")
    if args.share_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dpx.init(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group("gloo", rank=rank, world_size=world)

    algo_name, npairs, m, n, match, mismatch, gap_open, gap_extend, seed = WORKLOADS[args.workload]
    strong = npairs < 0  # negative = total over all ranks: each rank takes its contiguous ceil(N/G)-sized shard
    if strong and args.total_pairs:
        npairs = -args.total_pairs
    if strong:
        from dpx_gpu_genomics_project_amd.shard import shard_range
        lo, hi = shard_range(-npairs, rank, world)
        if (hi - lo) * world != -npairs:
            sys.exit(f"{args.workload}: {-npairs} pairs do not split evenly over {world} ranks")
        npairs = hi - lo
    if args.pairs:
        npairs = args.pairs
    algo = {"LNW": dpx.ALGO_LNW, "LSW": dpx.ALGO_LSW, "ANW": dpx.ALGO_ANW, "BSW": dpx.ALGO_BSW}[algo_name]
    # independent sub-batch per rank (weak scaling): same composition, different seed / pair indices
    if m == 0:
        from dpx_gpu_genomics_project_amd.synth import make_ragged_batch
        sb = make_ragged_batch(npairs, 80, 130, 100, 160, seed=seed + 1000 * rank)
    else:
        sb = dpx.make_batch(npairs, m, n, seed=seed + 1000 * rank, first_index=rank * npairs)
    # the resident batch is filled steps + warmup times: let the engine shop for a well-placed matrix pool
    batch = dpx.Batch(algo, sb.sequences, sb.pairs, match, mismatch, gap_open, gap_extend, band=BAND if algo_name == "BSW" else 0,
                      flags=dpx.TUNE_PLACEMENT)
    info = batch.info()
    # a dedicated (non-null) torch stream is made current: the fill kernel, the HIP events that time it and the
    # RCCL gather are all ordered on it
    tstream = torch.cuda.Stream(device=local_rank)
    torch.cuda.set_stream(tstream)
    stream = tstream.cuda_stream
    assert stream, "expected a non-null HIP stream handle"
    d_scores, _, _ = batch.device_results()
    scores_t = torch.as_tensor(_DevArray(d_scores, npairs), device=torch.device("cuda", local_rank))
    from dpx_gpu_genomics_project_amd.shard import gather_scores

    def exchange():
        if args.backend == "nccl":
            return gather_scores(scores_t, rank, world)  # RCCL over xGMI: 4 B x pairs per rank
        return gather_scores(scores_t.cpu(), rank, world)  # gloo rehearsal: host tensors

    def step():
        batch.fill(stream)  # async launch on torch's current stream
        if world > 1:
            return exchange()

    def fence():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # Device preconditioning (setup, untimed, not a step): after idle the chip needs ~80 ms of load before it holds its
    # steady clock -- the first ~20 fills of a process run ~4 % slower (tools/cold_start.py, profiles/README.md).  A fixed
    # 0.25 s of fills here makes the timed region measure sustained throughput whatever --warmup says.
    t_pre = time.perf_counter()
    precondition_fills = 0
    while time.perf_counter() - t_pre < 0.25:
        batch.fill(stream)
        torch.cuda.synchronize()
        precondition_fills += 1
    for _ in range(args.warmup):
        step()
    fence()
    # --full: HIP events around every timed fill for the per-kernel / roofline figures; a plain run launches the steps alone
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)] if args.full else None
    last = None
    t0 = time.perf_counter()
    for k in range(args.steps):
        if ev:
            ev[k][0].record()
        batch.fill(stream)
        if ev:
            ev[k][1].record()
        if world > 1:
            last = exchange()
    fence()
    elapsed = time.perf_counter() - t0

    red_dev = scores_t.device if args.backend == "nccl" else torch.device("cpu")
    t = torch.tensor([elapsed], dtype=torch.float64, device=red_dev)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())

    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, batch, algo_name, last.cpu().numpy() if last is not None else None)

    if args.full:
        kernel_ms = sum(a.elapsed_time(b) for a, b in ev) / args.steps
        local_kernel_ms = kernel_ms
        kt = torch.tensor([kernel_ms], dtype=torch.float64, device=red_dev)
        if world > 1:
            dist.all_reduce(kt, op=dist.ReduceOp.MAX)
        kernel_ms = float(kt.item())

    if args.full or args.dump_scores:
        scores, er, ec = batch.results()
    if args.full:
        # sanity on results (outside the timed region): a few pairs against the closed-form identical-pair score
        ident = [p for p in range(npairs) if (rank * npairs + p) % 101 == 100][:4]
        for p in ident if m else []:
            assert scores[p] == match * min(m, n), "identical pair must score match*len"
        # Every rank reports its own fill time, pool record and a checksum of its LOCAL scores; rank 0 checks the gathered vector
        # against every rank's checksum (not only its own slice), so the first run on N real GPUs verifies the collective itself.
        def checksum(vec) -> int:
            v = np.asarray(vec, dtype=np.int64)
            return int((v * (np.arange(v.size, dtype=np.int64) % 1021 + 1)).sum() & 0x7FFFFFFFFFFF)

        mine = {"rank": rank, "device": local_rank, "pairs": int(npairs), "kernel_ms": round(local_kernel_ms, 4),
                "pool": pool_record(batch.describe()), "scores_checksum": checksum(scores)}
        ranks = [mine]
        if world > 1:
            ranks = [None] * world
            dist.all_gather_object(ranks, mine)
        if world > 1 and rank == 0:  # the gathered vector must carry every rank's scores in rank order
            assert last is not None and last.numel() == sum(r["pairs"] for r in ranks)
            g = last.cpu().numpy()
            off = 0
            for r in ranks:
                r["gathered_ok"] = checksum(g[off:off + r["pairs"]]) == r["scores_checksum"]
                off += r["pairs"]
            assert torch.equal(last[:npairs].cpu(), torch.from_numpy(scores))
            assert all(r["gathered_ok"] for r in ranks), [r for r in ranks if not r["gathered_ok"]]

    if args.dump_scores:
        np.save(f"{args.dump_scores}.rank{rank}.npy", scores)
        if rank == 0 and world > 1:
            np.save(f"{args.dump_scores}.gathered.npy", last.cpu().numpy())

    if rank == 0:
        shape = f"{m}x{n}" if m else "short-read (reference 100-160 x query 80-130)"
        # arithmetic type of the kernel the engine picked for this batch (dpx_batch_describe): equal-shaped LSW/LNW pairs
        # whose query fits one stripe run two per wave on the packed-int16 pipe (v_pk_*_i16), everything else in int32
        desc = batch.describe()
        dtype = desc["dtype"]
        total_cells = info["cells"] * world
        value = total_cells * args.steps / elapsed / 1e9
        out = {
            "metric": "GCUPS", "value": round(value, 2), "unit": "GCUPS", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True,
            "scaling": "strong" if strong else "weak", "vs_baseline": None, "dtype": dtype, "data": "synthetic",
            "config": {"workload": f"{algo_name} {npairs}-pair {shape} batch per GPU, int16 score matrix written to HBM",
                       "algorithm": algo_name, "pairs_per_gpu": npairs, "query_len": m, "reference_len": n,
                       "match": match, "mismatch": mismatch, "gap": gap_open, "gap_extend": gap_extend if algo_name == "ANW" else None,
                       "parallelism": f"{world} rank(s), 1 per GPU, pairs sharded, RCCL gather of int32 scores" if world > 1 else "1 GPU",
                       "backend": dist.get_backend() if world > 1 else None, "world_size": dist.get_world_size() if world > 1 else 1,
                       "tune_placement": True,
                       "cells_per_gpu": info["cells"], "matrix_bytes_per_gpu": info["matrix_bytes"],
                       "precondition_fills": precondition_fills, "kernel": desc["kernel"],
                       "rows_per_lane": desc["rows_per_lane"]},
        }
        if args.full:
            achieved = info["algorithmic_bytes"] / (kernel_ms * 1e-3) / 1e9
            # HBM bytes per fill from the PMC passes of tools/profile_all.sh (rocprofv3 --pmc WRITE_SIZE / FETCH_SIZE, separate runs),
            # recorded together with a hash of the kernel sources: a figure measured on other kernels is reported as stale
            traffic, traffic_stale = None, None
            prof = os.path.join(ROOT, "profiles", "pmc_traffic.json")
            if os.path.exists(prof):
                try:
                    rec = json.load(open(prof))
                    traffic = rec.get("workloads", {}).get(args.workload)
                    traffic_stale = rec.get("kernel_source_sha256") != kernel_source_hash()
                except Exception:
                    traffic = None
            out["roofline"] = {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                               "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_stale": traffic_stale,
                               "kernel_ms": round(kernel_ms, 4), "algorithmic_bytes_per_launch": info["algorithmic_bytes"],
                               "kernel_gcups": round(info["cells"] / (kernel_ms * 1e-3) / 1e9, 1),
                               "pool": pool_record(desc)}
            # what a caller WITHOUT DPX_TUNE_PLACEMENT gets: the first pool the engine built (candidate 0 of the shopping), timed by the
            # engine with the same fill (3 launches) before the other candidates existed -- the product-representative figure beside the shopped one
            pool = out["roofline"]["pool"] or {}
            if pool.get("candidates_fill_ms"):
                first_ms = pool["candidates_fill_ms"][0]
                out["roofline"]["kernel_ms_first_pool"] = first_ms
                out["roofline"]["frac_first_pool"] = round(info["algorithmic_bytes"] / (first_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if first_ms > 0 else None
            if algo_name == "BSW":  # GCUPS counts refLen x queryLen as the reference does; also give the in-band rate
                inband = (info["algorithmic_bytes"] - npairs * (m + n + 28)) // 2
                out["roofline"]["in_band_cells_per_launch"] = inband
                out["roofline"]["in_band_kernel_gcups"] = round(inband / (kernel_ms * 1e-3) / 1e9, 1)
            out["ranks"] = ranks  # per rank: fill-kernel ms, matrix-pool record, checksum of its scores (+ gathered_ok on rank 0's check)
            if not args.no_cpu_baseline and world == 1:
                out["cpu_baseline"] = cpu_baseline(sb, algo_name, match, mismatch, gap_open, gap_extend,
                                                   args.cpu_pairs if m else npairs, shape)
        print(json.dumps(out), flush=True)
    batch.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
