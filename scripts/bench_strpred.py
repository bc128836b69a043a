"""kernel_ns per step of the LIKE-family window modes, relative to plain
`contains` measured in the same run.

  python scripts/bench_strpred.py [--rows 100000000] [--steps 10] [--warmup 3]

Uses the same c3b shard bench.py --workload c3s generates (and reuses it when
present): SELECT count(*) WHERE message <op> 'error'. Each op gets its own
plan. A throwaway plan runs first and fills the hot tier, so every measured
plan finds its decompressed chunk images resident and none of them pays for
decompression; the figure compared is kernel_ns - decomp_ns per step (def
levels + predicate kernels + the count). Prints one JSON line."""

import argparse
import json
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OPS = ["contains", "icontains", "starts_with", "ends_with", "not_contains"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--needle", default="error")
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

    shard = os.path.join(a.data_dir, f"c3s_{a.rows}_r0")
    stream_dir = os.path.join(shard, "stream")
    if not os.path.exists(os.path.join(stream_dir, "stream.json")):
        workers = max(8, min(len(os.sched_getaffinity(0)),
                             int(os.environ.get("OMP_NUM_THREADS", "1024"))))
        gen_stream(shard, "stream", "c3b", rows=a.rows, seed=42,
                   workers=workers)

    session = GpuSession(device_mask=1)
    provider = StandardTableProvider(stream_dir, session)
    res = {}
    warm = provider.scan({"select": [{"agg": "count_star"}], "preds": [
        {"col": "message", "op": "contains", "lit": a.needle}]})
    warm.execute(0)
    warm.close()
    for op in OPS:
        q = {"select": [{"agg": "count_star"}],
             "preds": [{"col": "message", "op": op, "lit": a.needle}]}
        plan = provider.scan(q)
        plan.load()
        for _ in range(a.warmup):
            plan.execute(0)
        m0 = plan.metrics()
        for _ in range(a.steps):
            batch = plan.execute(0)
        m1 = plan.metrics()
        res[op] = {
            "kernel_ms_per_step": round(
                ((m1["kernel_ns"] - m0["kernel_ns"])
                 - (m1["decomp_ns"] - m0["decomp_ns"])) / a.steps / 1e6, 4),
            "cache_hit_frac": round(
                m1["cache_hit_bytes"] / max(m1["bytes_scanned"], 1), 4),
            "decomp_ms_per_step": round(
                (m1["decomp_ns"] - m0["decomp_ns"]) / a.steps / 1e6, 4),
            "count": batch.column(0).to_pylist()[0],
        }
        plan.close()
    base = res["contains"]["kernel_ms_per_step"]
    for op in OPS:
        res[op]["ratio_to_contains"] = round(
            res[op]["kernel_ms_per_step"] / base, 4)
    print(json.dumps({"rows": a.rows, "needle": a.needle, "steps": a.steps,
                      "ops": res}))


if __name__ == "__main__":
    main()
