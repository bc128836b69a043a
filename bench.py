#!/usr/bin/env python3
"""Benchmark for the MI355X query path (BASELINE.json metric: rows/sec +
GB/s scanned for SELECT...WHERE...GROUP BY over a Parseable log stream).

Contract (driver): `python bench.py --gpus N --steps K --warmup W`, launched
for N>1 via torch.distributed.run with one rank per GPU (RCCL). A "step" is
one pass of the hot path (LZ4_RAW decompress -> decode -> filter -> hash
group-by -> cross-rank RCCL merge) over this rank's shard, with raw column
chunks already resident in HBM when the timed region starts (plan.load() is
untimed; the first-touch cost is reported as config.load_s / plan_build_s
and the PCIe-inclusive rate as load_gbps_pcie — see DESIGN.md §5). Weak
scaling: each rank generates and scans its own DISTINCT full-size shard
(seed = 42 + rank) so cross-rank key spaces diverge like real per-minute
shards do; the RCCL merge reduces the union key space.

Default workload: the BASELINE metric's own shape — SELECT host,count(*),
max(latency) WHERE ts BETWEEN ... GROUP BY host (BASELINE.json configs[2],
run per-GPU; the BETWEEN selects ~50% of row groups). `--workload
c1|c3s|c4s` run the other BASELINE shapes at --rows scale.

A plain run does only what the headline figure needs: generate the shard
(once per data dir), build + load the plan, warm up, time the steps, print
the line. It runs at 100 M rows/GPU so that set-up (datagen + plan build)
stays within seconds even with few host cores. `--full` adds the legs that take runs of their own (the
hot-tier repeat query and the CPU-oracle baseline) and defaults to the
metric's stated 1 B-row scale, as every figure in BASELINE.md/DESIGN.md.

`--dump-outputs DIR` writes the final table the last timed step returned
(what a caller of plan.execute + DistMerger.step receives) as
DIR/<name>.npy, one float array per key/aggregate column in row order.
Shards are seeded (42 + rank), so the same arguments give the same inputs
and two builds can be compared output for output.

Rank 0 prints ONE JSON line."""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # 8 TB/s spec (MI355X_MICROARCH.md)


WORKLOADS = {
    # name -> (datagen config, query builder)
    "c1": ("c1", lambda a: {
        "select": [{"agg": "count_star"}],
        "group_by": ["level"],
    }),
    "c2s": ("c1", lambda a: {   # the BASELINE c2 shape, per-GPU scale
        "select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"}],
        "group_by": ["host"],
        "preds": [{"col": "p_timestamp", "op": "between",
                   "lo": 1756684800000, "hi": 1756684800000 + (
                       a.between_ms or  # default: ~50% of row groups
                       ((args_n_files(a) + 1) // 2) * 60_000)}],
    }),
    "c3s": ("c3b", lambda a: {  # the BASELINE c3 shape (1B LIKE byte scan);
                                # slim schema (ts+message) so the 1B stream
                                # fits the GPU box's local disk
        "select": [{"agg": "count_star"}],
        "preds": [{"col": "message", "op": "contains", "lit": "error"}],
    }),
    "c4s": ("c4", lambda a: {   # c4-shaped: OTel 64 sparse cols, 3-key group-by
        "select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"},
                   {"agg": "sum", "col": "attr_i0"}],
        "group_by": ["service", "span_kind", "status"],
        "preds": [{"col": "attr_i1", "op": "ge", "lit": 200_000}],
    }),
}


def args_n_files(a):
    return (a.rows + 262_143) // 262_144


def host_cpus():
    """CPUs this process may actually use: the affinity mask, further capped
    by OMP_NUM_THREADS where a job scheduler sets it (a container quota does
    not show in os.cpu_count())."""
    try:
        n = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        n = os.cpu_count() or 8
    try:
        n = min(n, int(os.environ["OMP_NUM_THREADS"]))
    except (KeyError, ValueError):
        pass
    return max(n, 1)


def dump_outputs(out_dir, rows, query):
    """Write the final result table column by column as <name>.npy.
    Numeric columns -> float64 (None -> NaN; counts and the int64 aggregates
    of the bench workloads are far below 2**53, so exact). String columns ->
    float32 [n_rows, max_len] of zero-padded UTF-8 bytes (None -> all -1),
    so a swapped or missing group key shows up as a numeric difference."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    names = []
    for k, g in enumerate(query.get("group_by", [])):
        g = g if isinstance(g, str) else "bin_" + g["bin"]
        names.append(f"key{k}_{g}")
    for i, a in enumerate(query["select"]):
        names.append(f"agg{i}_{a['agg']}" + (f"_{a['col']}" if "col" in a else ""))
    for c, name in enumerate(names):
        col = [r[c] for r in rows]
        if any(isinstance(v, str) for v in col):
            enc = [None if v is None else v.encode() for v in col]
            width = max((len(b) for b in enc if b is not None), default=0)
            arr = np.zeros((len(col), width), dtype=np.float32)
            for r, b in enumerate(enc):
                if b is None:
                    arr[r, :] = -1.0
                else:
                    arr[r, :len(b)] = np.frombuffer(b, dtype=np.uint8)
        else:
            arr = np.array([np.nan if v is None else float(v) for v in col],
                           dtype=np.float64)
        np.save(os.path.join(out_dir, name + ".npy"), arr)


def log(msg):
    if int(os.environ.get("RANK", "0")) == 0:
        print(msg, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="c2s")
    ap.add_argument("--rows", type=int, default=None,
                    help="rows per GPU (weak scaling); default 100M, or "
                    "with --full the 1B that BASELINE quotes")
    ap.add_argument("--full", action="store_true",
                    help="also run the legs that take runs of their own: "
                    "the hot-tier repeat query and the CPU-oracle baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's result table as "
                    "DIR/<name>.npy")
    ap.add_argument("--between-ms", type=int, default=0,
                    help="c2s: BETWEEN window width (default ~50%% of range)")
    ap.add_argument("--data-dir", default=None,
                    help="default: $GPUQ_DATA, else /dev/shm when large "
                    "(the 8-rank 1B shards exceed small /tmp overlays)")
    ap.add_argument("--gen-workers", type=int, default=0)
    ap.add_argument("--skip-cpu-baseline", action="store_true")
    ap.add_argument("--skip-hot-tier", action="store_true",
                    help="skip the repeat-query leg (PMC profiling passes "
                    "must not mix cold and cache-served launches)")
    ap.add_argument("--cpu-baseline-full", action="store_true",
                    help="time the oracle over the FULL stream (all files, "
                    "all cores) instead of the bounded sample — the "
                    "once-per-round measured baseline (BASELINE.md)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.rows is None:
        args.rows = 1_000_000_000 if args.full else 100_000_000

    if args.data_dir is None:
        args.data_dir = os.environ.get("GPUQ_DATA")
    if args.data_dir is None:
        import shutil

        try:
            big_shm = shutil.disk_usage("/dev/shm").free > 200e9
        except OSError:
            big_shm = False
        args.data_dir = "/dev/shm/gpuq_bench" if big_shm else "/tmp/gpuq_bench"

    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    distributed = world > 1
    if distributed:
        import datetime
        # generous timeout: rank 0 may spend minutes in datagen before the
        # first collective on a fresh box
        dist.init_process_group("nccl", timeout=datetime.timedelta(minutes=60))
        torch.cuda.set_device(local_rank)
        merge_dev = f"cuda:{local_rank}"
    else:
        merge_dev = "cpu"

    from datagen.gen import gen_stream
    from parseable_amd import GpuSession, StandardTableProvider
    from parseable_amd.dist import DistMerger

    cfg, qbuild = WORKLOADS[args.workload]
    query = qbuild(args)

    # --- shard (DISTINCT content per rank: seed = 42 + rank) ---
    n_files = args_n_files(args)
    shard = os.path.join(args.data_dir, f"{args.workload}_{args.rows}_r{rank}")
    stream_dir = os.path.join(shard, "stream")
    workers = args.gen_workers or max(8, host_cpus() // world)
    # cap per-rank host planning threads too (8 ranks x all-core threads thrash)
    os.environ.setdefault("GPUQ_HOST_THREADS", str(workers))
    if not os.path.exists(os.path.join(stream_dir, "stream.json")):
        log(f"[bench] generating {args.rows} rows/rank ({n_files} files, "
            f"{workers} workers/rank) under {shard} ...")
        t0 = time.time()
        gen_stream(shard, "stream", cfg, rows=args.rows, seed=42 + rank,
                   workers=workers)
        log(f"[bench] datagen took {time.time() - t0:.1f}s")
    if distributed:
        dist.barrier()

    # --- plan build + HBM residency (untimed; first-touch cost reported) ---
    session = GpuSession(device_mask=1 << local_rank)
    provider = StandardTableProvider(stream_dir, session)
    t0 = time.time()
    plan = provider.scan(query)
    plan_s = time.time() - t0
    t0 = time.time()
    plan.load()
    load_s = time.time() - t0
    log(f"[bench] plan built in {plan_s:.1f}s, loaded to HBM in {load_s:.1f}s")

    merger = DistMerger(query, device=merge_dev)
    first = plan.execute(0)
    merger.setup(first)

    # --- warmup ---
    for _ in range(args.warmup):
        merger.step(plan.execute(0))

    m_before = plan.metrics()

    # --- timed region ---
    if distributed:
        dist.barrier()
    torch.cuda.synchronize() if torch.cuda.is_available() else None
    t_start = time.perf_counter()
    rows_final = None
    for _ in range(args.steps):
        batch = plan.execute(0)
        rows_final = merger.step(batch)
    torch.cuda.synchronize() if torch.cuda.is_available() else None
    if distributed:
        dist.barrier()
    elapsed = time.perf_counter() - t_start
    if distributed:
        t = torch.tensor([elapsed], dtype=torch.float64, device=merge_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    m_after = plan.metrics()

    # --- per-step aggregates over all ranks ---
    rank_rows = m_after["rows_scanned"]  # rows per execute on this rank
    rank_bytes = m_after["bytes_scanned"]
    rank_rg_bytes = m_after["rowgroup_bytes_total"]
    if distributed:
        t = torch.tensor([rank_rows, rank_bytes, rank_rg_bytes],
                         dtype=torch.float64, device=merge_dev)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        total_rows, total_bytes, total_rg_bytes = (float(x) for x in t.tolist())
    else:
        total_rows, total_bytes, total_rg_bytes = (
            float(rank_rows), float(rank_bytes), float(rank_rg_bytes))

    sec_per_step = elapsed / args.steps
    rows_per_sec = total_rows / sec_per_step
    gbps_scanned = total_bytes / sec_per_step / 1e9
    gbps_rowgroup = total_rg_bytes / sec_per_step / 1e9

    # --- kernel-stage breakdown (this rank; HIP events inside libgpuq) ---
    dk = (m_after["kernel_ns"] - m_before["kernel_ns"]) / args.steps
    dd = (m_after["decomp_ns"] - m_before["decomp_ns"]) / args.steps
    raw_b = rank_bytes  # compressed chunk bytes resident in HBM, read once/step
    # decompressed arena bytes: est = hbm_bytes_est - raw - dec (we stored raw+2*dec)
    dec_b = (m_after["hbm_bytes_est"] - raw_b) / 2
    # Algorithmic bytes per launch, per workload (constants documented in
    # DESIGN.md §3/§5):
    #  - lz4 sweep: compressed read + decompressed write
    #  - c1 fused dict-count: decompressed pages read once (no materialization)
    #  - c2s: dec read + latency val write+read (8B x2) + valid w+r (1x2) +
    #    gid w+r (4B x2) + mask read (1); the ts BETWEEN is chunk-stats
    #    elided for fully-covered row groups (pred_all_true), so ts decode
    #    and cmp touch only boundary row groups (~0 B/row at 1B scale)
    #  - c3s: dec read (values scanned from LDS windows) + mask write
    decomp_algo_bytes = raw_b + dec_b
    other_ns = max(dk - dd, 1.0)
    decode_algo_bytes = {
        "c1": dec_b,
        "c2s": dec_b + rank_rows * (2 * 8 + 2 * 1 + 2 * 4 + 1),
        "c3s": dec_b + rank_rows * 1,
        "c4s": dec_b + rank_rows * (3 * 16 + 3 * 4 + 4 + 3),
    }[args.workload]
    decode_kernel = {
        "c1": "dict_count_fused",
        "c2s": "decode+filter+groupby",
        "c3s": "bytes_contains(LIKE)",
        "c4s": "decode+filter+groupby",
    }[args.workload]
    if dd >= other_ns:
        roof_kernel, roof_bytes, roof_ns = "lz4_page_decompress", decomp_algo_bytes, dd
    else:
        roof_kernel, roof_bytes, roof_ns = decode_kernel, decode_algo_bytes, other_ns
    achieved_gbs = roof_bytes / max(roof_ns, 1.0)  # bytes/ns == GB/s
    traffic = None  # measured HBM bytes/launch from rocprofv3 --pmc passes
    try:
        with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as fh:
            t = json.load(fh)["traffic"].get(args.workload, {})
        # per-launch traffic is scale-specific: only quote it when the PMC
        # pass ran at this row count
        if t.get("rows", args.rows) == args.rows:
            traffic = t.get(roof_kernel)
            if traffic is not None:
                traffic = round(traffic)
    except Exception:
        pass
    roofline = {
        "bound": "hbm",
        "kernel": roof_kernel,
        "achieved": round(achieved_gbs, 2),
        "peak": HBM_PEAK_GBS,
        "unit": "GB/s",
        "frac": round(achieved_gbs / HBM_PEAK_GBS, 4),
        "traffic": traffic,  # rocprofv3 --pmc (profiles/r01_pmc_summary.md);
                             # measured on the same workload at --rows 1e8/3e7
    }

    # the first plan's HBM is released before the repeat-query plan exists:
    # peak device memory stays one plan + the hot tier
    plan.close()
    hot_tier = None
    if args.full and not args.skip_hot_tier:

    # --- hot-tier repeat query: a NEW plan over the same
    # chunks, served from the session cache — no raw re-upload, no LZ4 walk,
    # no decompression. Local to each rank (no collectives); rank 0 reports.
        t0 = time.time()
        plan2 = provider.scan(query)
        plan2_s = time.time() - t0
        t0 = time.time()
        plan2.load()
        load2_s = time.time() - t0
        for _ in range(2):
            plan2.execute(0)
        m2a = plan2.metrics()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            plan2.execute(0)
        torch.cuda.synchronize() if torch.cuda.is_available() else None
        hot_elapsed = time.perf_counter() - t0
        m2b = plan2.metrics()
        hot_tier = {
            "ms_per_step": round(hot_elapsed / args.steps * 1e3, 3),
            "rows_per_sec": round(rank_rows / (hot_elapsed / args.steps), 1),
            "gb_per_sec_scanned": round(
                rank_bytes / (hot_elapsed / args.steps) / 1e9, 2),
            "decomp_ms_per_step": round(
                (m2b["decomp_ns"] - m2a["decomp_ns"]) / args.steps / 1e6, 3),
            "cache_hit_frac": round(
                m2b["cache_hit_bytes"] / max(m2b["bytes_scanned"], 1), 4),
            "first_touch_s": round(plan2_s + load2_s, 2),
        }
        plan2.close()

    # --- CPU baseline: the oracle (kind=port) on a bounded sample ---
    cpu_baseline = None
    if args.full and rank == 0 and world == 1 and not args.skip_cpu_baseline:
        from oracle import query_oracle as qo
        import pyarrow as pa

        all_files = sorted(
            os.path.join(dp, f)
            for dp, _, fs in os.walk(stream_dir)
            for f in fs if f.endswith(".parquet")
        )
        # bounded sample (~10-30s of CPU work) by default; --cpu-baseline-full
        # runs the whole stream once per round (the measured, not
        # extrapolated, figure for BASELINE.md)
        if args.cpu_baseline_full:
            sample_files = all_files
        else:
            sample_files = all_files[: max(2, min(256, n_files // 8))]
        import pyarrow.parquet as pq

        sample_rows = sum(pq.read_metadata(f).num_rows for f in sample_files)
        tcb = time.perf_counter()
        qo.execute(sample_files, query)
        tcb = time.perf_counter() - tcb
        cpu_baseline = {
            "value": round(sample_rows / tcb, 1),
            "unit": "rows/s",
            "cores": pa.cpu_count(),
            "kind": "port",
            "sample": ("FULL stream: " if args.cpu_baseline_full else "") +
                      f"oracle (pyarrow-decode + numpy agg) on {len(sample_files)} "
                      f"files = {sample_rows} rows, {tcb:.1f}s",
        }

    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, rows_final, query)

    if rank == 0:
        out = {
            "metric": "rows/sec scanned (SELECT...WHERE...GROUP BY, Parseable parquet dialect)",
            "value": round(rows_per_sec, 1),
            "unit": "rows/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(sec_per_step * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,  # no published reference numbers
            "dtype": "int64",
            "data": "synthetic",
            "config": {
                "workload": args.workload,
                "query": {
                    "c1": "SELECT level,count(*) GROUP BY level",
                    "c2s": "SELECT host,count(*),max(latency) WHERE ts BETWEEN ... GROUP BY host",
                    "c3s": "SELECT count(*) WHERE message LIKE '%error%'",
                    "c4s": "SELECT service,span_kind,status,count(*),max(latency),sum(attr_i0) WHERE attr_i1>=200000 GROUP BY 1,2,3",
                }[args.workload],
                "rows_per_gpu": args.rows,
                "files_per_gpu": n_files,
                "rank_shards": "distinct content per rank (seed = 42 + rank)",
                "parallelism": f"dp{world}",
                "gb_per_sec_scanned": round(gbps_scanned, 2),
                "gb_per_sec_rowgroup_bytes": round(gbps_rowgroup, 2),
                "kernel_ms_per_step": round(dk / 1e6, 3),
                "decomp_ms_per_step": round(dd / 1e6, 3),
                "plan_build_s": round(plan_s, 2),
                "load_s": round(load_s, 2),
                "load_gbps_pcie": round(
                    rank_bytes / max(m_after["load_ns"], 1), 2),
                "hot_tier_repeat": hot_tier,
            },
            "roofline": roofline,
            "cpu_baseline": cpu_baseline,
        }
        print(json.dumps(out), flush=True)
        if rows_final is not None:
            log(f"[bench] result rows (first 8): {rows_final[:8]}")

    if distributed:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
