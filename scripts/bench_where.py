"""kernel_ns per step of OR groups against their single-leaf queries, measured
in the same run on the same build.

  python scripts/bench_where.py [--rows 100000000] [--steps 10] [--warmup 3]
                                [--cases 1,2,3]

Case 1 (folded into one LUT):  level = 'ERROR'; level = 'WARN'; the OR.
Case 2 (general path, acc/tmp): message contains 'error'; contains
                                'timeout'; the OR.
Case 3 (numeric, general path): latency < 100000; f_i64 > 2^39; the OR.

Case 2 runs on the c3b shard bench.py --workload c3s generates, cases 1 and 3
on the c1 shard of the default c2s workload (c3b has no level or numeric
value column); both are reused when present. Every query is SELECT count(*).
A throwaway plan per shard fills the hot tier, so every measured plan finds
its decompressed chunk images resident; the figure compared is kernel_ns -
decomp_ns per step (def levels + predicate kernels + mask combines + the
count). Per case the script reports the OR against the sum of its leaves,
and against the AND of the same leaves — the same leaf launches into one mask
without combine passes, so the difference is what the memsets and the two
combine kernels cost. Prints one JSON line."""

import argparse
import json
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def L(col, op, lit):
    return {"col": col, "op": op, "lit": lit}


CASES = {
    1: ("c2s", "c1", "level", [L("level", "eq", "ERROR"), L("level", "eq", "WARN")]),
    2: ("c3s", "c3b", "message", [L("message", "contains", "error"),
                                  L("message", "contains", "timeout")]),
    3: ("c2s", "c1", "latency", [L("latency", "lt", 100_000),
                                 L("f_i64", "gt", 1 << 39)]),
}


def measure(provider, query, steps, warmup):
    plan = provider.scan(query)
    plan.load()
    for _ in range(warmup):
        plan.execute(0)
    m0 = plan.metrics()
    for _ in range(steps):
        batch = plan.execute(0)
    m1 = plan.metrics()
    out = {
        "kernel_ms_per_step": round(
            ((m1["kernel_ns"] - m0["kernel_ns"])
             - (m1["decomp_ns"] - m0["decomp_ns"])) / steps / 1e6, 4),
        "cache_hit_frac": round(
            m1["cache_hit_bytes"] / max(m1["bytes_scanned"], 1), 4),
        "count": batch.column(0).to_pylist()[0],
    }
    plan.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="1,2,3")
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

    session = GpuSession(device_mask=1)
    providers = {}
    res = {}
    count = [{"agg": "count_star"}]
    for case in (int(c) for c in a.cases.split(",")):
        workload, cfg, warm_col, leaves = CASES[case]
        if workload not in providers:
            shard = os.path.join(a.data_dir, f"{workload}_{a.rows}_r0")
            stream_dir = os.path.join(shard, "stream")
            if not os.path.exists(os.path.join(stream_dir, "stream.json")):
                workers = max(8, min(len(os.sched_getaffinity(0)),
                                     int(os.environ.get("OMP_NUM_THREADS", "1024"))))
                gen_stream(shard, "stream", cfg, rows=a.rows, seed=42,
                           workers=workers)
            providers[workload] = StandardTableProvider(stream_dir, session)
        provider = providers[workload]
        # fill the hot tier with every column the case reads
        warm = provider.scan({"select": count, "preds": leaves})
        warm.execute(0)
        warm.close()
        r = {"leaves": [measure(provider, {"select": count, "preds": [p]},
                                a.steps, a.warmup) for p in leaves],
             "and": measure(provider, {"select": count, "preds": leaves},
                            a.steps, a.warmup),
             "or": measure(provider, {"select": count, "where": {"or": leaves}},
                           a.steps, a.warmup)}
        s = sum(x["kernel_ms_per_step"] for x in r["leaves"])
        r["sum_of_leaves_ms"] = round(s, 4)
        r["or_over_sum"] = round(r["or"]["kernel_ms_per_step"] / s, 4)
        r["or_minus_and_ms"] = round(r["or"]["kernel_ms_per_step"]
                                     - r["and"]["kernel_ms_per_step"], 4)
        res[f"case{case}"] = r
    print(json.dumps({"rows": a.rows, "steps": a.steps, "cases": res}))


if __name__ == "__main__":
    main()
