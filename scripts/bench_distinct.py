"""kernel_ns per step of COUNT(DISTINCT) on the c2 data, next to the query a
caller had to run before the op existed.

  python scripts/bench_distinct.py [--rows 100000000] [--steps 10] [--warmup 3]
                                   [--bitmap-bits 67108864,268435456,1073741824]

Uses the same c1-config shard bench.py (workload c2s) generates, and reuses it
when present. Each case gets its own plan; a throwaway plan per column set
fills the hot tier first, so every measured plan finds its decompressed chunk
images resident and the figure compared is kernel_ns - decomp_ns per step.
The path each distinct agg took is read from the plan debug line of one
extra, untimed execute. Cases:

  level_by_host          count(distinct level) GROUP BY host  (bitmap via LDS)
  level_by_host_global   the same with GPUQ_DISTINCT_LDS_BITS=0 (no LDS copy)
  level_by_host_hash     the same with GPUQ_DISTINCT_FORCE_HASH=1
  host                   count(distinct host)
  host_global            the same with GPUQ_DISTINCT_LDS_BITS=0
  latency                count(distinct latency)        (~10^6 values; bitmap)
  latency_hash           the same, forced onto the hash set
  groupby_host_level     count(*) GROUP BY host, level — the same information
                         without the op

--bitmap-bits runs `host_by_latency_5pct` (count(distinct host) GROUP BY
latency over a ~5 % time window: ~10^6 groups x 1024 padded values, just
under 2^30 bits, ~5 M pairs) once per GPUQ_DISTINCT_BITMAP_BITS value: the
one shape of this data whose path depends on the threshold. Prints one JSON
line."""

import argparse
import json
import os
import re
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASE_TS = 1756684800000
ROWS_PER_FILE = 262_144   # one file per minute


def cd(col):
    return {"agg": "count_distinct", "col": col}


CASES = {
    "level_by_host": ({"select": [cd("level")], "group_by": ["host"]}, {}),
    "level_by_host_global": ({"select": [cd("level")], "group_by": ["host"]},
                             {"GPUQ_DISTINCT_LDS_BITS": "0"}),
    "level_by_host_hash": ({"select": [cd("level")], "group_by": ["host"]},
                           {"GPUQ_DISTINCT_FORCE_HASH": "1"}),
    "host": ({"select": [cd("host")]}, {}),
    "host_global": ({"select": [cd("host")]}, {"GPUQ_DISTINCT_LDS_BITS": "0"}),
    "latency": ({"select": [cd("latency")]}, {}),
    "latency_hash": ({"select": [cd("latency")]},
                     {"GPUQ_DISTINCT_FORCE_HASH": "1"}),
    "groupby_host_level": ({"select": [{"agg": "count_star"}],
                            "group_by": ["host", "level"]}, {}),
}


def stderr_of(fn):
    """fn() with fd 2 redirected to a file -> (fn's result, the text): the
    library writes the plan debug lines with fprintf."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as tf:
        os.dup2(tf.fileno(), 2)
        try:
            result = fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tf.seek(0)
        return result, tf.read().decode(errors="replace")


def measure(provider, q, env, steps, warmup):
    os.environ.update(env)
    os.environ["GPUQ_PLAN_DEBUG"] = "1"
    try:
        plan, dbg = stderr_of(lambda: provider.scan(dict(q)))
    finally:
        os.environ.pop("GPUQ_PLAN_DEBUG", None)
        for k in env:
            os.environ.pop(k, None)
    try:
        plan.load()
        dbg += stderr_of(lambda: plan.execute(0))[1]
        for _ in range(warmup):
            plan.execute(0)
        m0 = plan.metrics()
        for _ in range(steps):
            batch = plan.execute(0)
        m1 = plan.metrics()
    finally:
        plan.close()
    nk = len(q.get("group_by", []))
    out = {
        "kernel_ms_per_step": round(
            ((m1["kernel_ns"] - m0["kernel_ns"])
             - (m1["decomp_ns"] - m0["decomp_ns"])) / steps / 1e6, 4),
        "decomp_ms_per_step": round(
            (m1["decomp_ns"] - m0["decomp_ns"]) / steps / 1e6, 4),
        "cache_hit_frac": round(
            m1["cache_hit_bytes"] / max(m1["bytes_scanned"], 1), 4),
        "groups_out": batch.num_rows,
        "agg0_total": sum(batch.column(nk + 1).to_pylist()),
    }
    m = re.search(r"distinct agg=0 col=\S+ path=(\S+) groups=(\d+) card=(\d+) "
                  r"pairs=(\d+)(?: mark=(\S+))?", dbg)
    if m:
        out.update(path=m.group(1), groups=int(m.group(2)),
                   card=int(m.group(3)), pairs=int(m.group(4)))
        if m.group(5):
            out["mark"] = m.group(5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bitmap-bits", default="",
                    help="comma-separated GPUQ_DISTINCT_BITMAP_BITS values")
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

    session = GpuSession(device_mask=1)
    provider = StandardTableProvider(stream_dir, session)
    # fill the hot tier: dict-gid images of host / level, values of latency
    # and p_timestamp
    warm = provider.scan({
        "select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"}],
        "group_by": ["host", "level"],
        "preds": [{"col": "p_timestamp", "op": "ge", "lit": BASE_TS + 1}]})
    warm.execute(0)
    warm.close()

    res = {"rows": a.rows, "steps": a.steps, "cases": {}}
    for name, (q, env) in CASES.items():
        res["cases"][name] = measure(provider, q, env, a.steps, a.warmup)
    if a.bitmap_bits:
        n_files = (a.rows + ROWS_PER_FILE - 1) // ROWS_PER_FILE
        hi = BASE_TS + max(1, n_files // 20) * 60_000
        q = {"select": [cd("host")], "group_by": ["latency"],
             "time_range": [BASE_TS, hi]}
        res["host_by_latency_5pct"] = {}
        for bits in a.bitmap_bits.split(","):
            res["host_by_latency_5pct"][bits] = measure(
                provider, q, {"GPUQ_DISTINCT_BITMAP_BITS": bits}, a.steps,
                a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
