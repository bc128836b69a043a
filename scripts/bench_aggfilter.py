"""One filtered scan against the two scans it replaces, and k_agg_fcount
against k_agg<.., true>, on the c2 data.

  python scripts/bench_aggfilter.py [--rows 100000000] [--steps 10]
                                    [--warmup 3] [--runs 5] [--modes ...]

The error-rate shape under the c2 time range (bench.py's c2s BETWEEN):

  filtered   host, count(*), count(*) FILTER (WHERE level = 'ERROR')
  nofcount   the same plan built under GPUQ_NO_FCOUNT=1 (k_agg<.., true>)
  twoscans   what a build without filters needs for the same answer:
             count(*) BY host, and count(*) BY host with level = 'ERROR' in
             WHERE — the figure is the sum of the two

`twoscans` uses nothing of the filter feature, so this script, run from a
checkout of an older commit with --modes twoscans, measures that commit. Runs
the c1 shard of bench.py's c2s workload (reused when present). Per run a fresh
plan is built, loaded, warmed and timed: ms_per_step is wall time around
execute(), kernel_ms_per_step the HIP-event time less decompression. Prints
one JSON line with every run and min / median / max per mode."""

import argparse
import json
import os
import shutil
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASE = 1756684800000
STAR = {"agg": "count_star"}
ERR = {"col": "level", "op": "eq", "lit": "ERROR"}


def measure(provider, query, steps, warmup, env=None):
    os.environ.update(env or {})
    try:
        plan = provider.scan(query)
    finally:
        for k in env or {}:
            os.environ.pop(k, None)
    plan.load()
    for _ in range(warmup):
        plan.execute(0)
    m0 = plan.metrics()
    t0 = time.perf_counter()
    for _ in range(steps):
        batch = plan.execute(0)
    wall = time.perf_counter() - t0
    m1 = plan.metrics()
    out = {
        "ms_per_step": round(wall / steps * 1e3, 3),
        "kernel_ms_per_step": round(
            ((m1["kernel_ns"] - m0["kernel_ns"])
             - (m1["decomp_ns"] - m0["decomp_ns"])) / steps / 1e6, 3),
        "groups": batch.num_rows,
        "checksum": [sum(batch.column(i).to_pylist())
                     for i in range(2, batch.num_columns, 2)],
    }
    plan.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--modes", default="filtered,nofcount,twoscans")
    ap.add_argument("--data-dir", default=os.environ.get("GPUQ_DATA"))
    a = ap.parse_args()
    if a.data_dir is None:
        try:
            big_shm = shutil.disk_usage("/dev/shm").free > 200e9
        except OSError:
            big_shm = False
        a.data_dir = "/dev/shm/gpuq_bench" if big_shm else "/tmp/gpuq_bench"

    from datagen.gen import gen_stream
    from parseable_amd import GpuSession, StandardTableProvider

    shard = os.path.join(a.data_dir, f"c2s_{a.rows}_r0")
    stream_dir = os.path.join(shard, "stream")
    if not os.path.exists(os.path.join(stream_dir, "stream.json")):
        workers = max(8, min(len(os.sched_getaffinity(0)),
                             int(os.environ.get("OMP_NUM_THREADS", "1024"))))
        gen_stream(shard, "stream", "c1", rows=a.rows, seed=42, workers=workers)
    n_files = (a.rows + 262_143) // 262_144
    window = [{"col": "p_timestamp", "op": "between", "lo": BASE,
               "hi": BASE + ((n_files + 1) // 2) * 60_000}]
    session = GpuSession(device_mask=1)
    provider = StandardTableProvider(stream_dir, session)
    # fill the hot tier with every column the shape reads
    warm = provider.scan({"select": [STAR], "group_by": ["host"],
                          "preds": window + [ERR]})
    warm.execute(0)
    warm.close()

    filtered = {"select": [STAR, dict(STAR, filter=ERR)], "group_by": ["host"],
                "preds": window}
    scans = [{"select": [STAR], "group_by": ["host"], "preds": window},
             {"select": [STAR], "group_by": ["host"], "preds": window + [ERR]}]
    res = {m: [] for m in a.modes.split(",")}
    for _ in range(a.runs):
        for mode in res:   # modes alternate inside a run
            if mode == "filtered":
                r = measure(provider, filtered, a.steps, a.warmup)
            elif mode == "nofcount":
                r = measure(provider, filtered, a.steps, a.warmup,
                            {"GPUQ_NO_FCOUNT": "1"})
            else:
                two = [measure(provider, q, a.steps, a.warmup) for q in scans]
                r = {"ms_per_step": round(sum(x["ms_per_step"] for x in two), 3),
                     "kernel_ms_per_step": round(
                         sum(x["kernel_ms_per_step"] for x in two), 3),
                     "groups": [x["groups"] for x in two],
                     "checksum": [x["checksum"] for x in two]}
            res[mode].append(r)
    summary = {}
    for mode, runs in res.items():
        for k in ("ms_per_step", "kernel_ms_per_step"):
            v = [r[k] for r in runs]
            summary[f"{mode}.{k}"] = {"min": min(v),
                                      "median": statistics.median(v),
                                      "max": max(v)}
    print(json.dumps({"rows": a.rows, "steps": a.steps, "runs": a.runs,
                      "summary": summary, "runs_detail": res}))


if __name__ == "__main__":
    main()
