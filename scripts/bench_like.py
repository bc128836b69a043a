"""kernel_ns per step of the general LIKE / ILIKE pattern ops next to plain
`contains`, measured in the same run.

  python scripts/bench_like.py [--rows 100000000] [--steps 10] [--warmup 3]
                               [--runs 5] [--cases op:literal ...]

Uses the same c3b shard bench.py --workload c3s generates (and reuses it when
present): SELECT count(*) WHERE message <op> '<literal>'. Default cases:

  contains:error        the tuned k_contains_win<> path
  like:%error%          canonicalised — must build the contains plan
  like:%error%a%        general, one inner '%', first literal `error`
  ilike:%error%a%       the same, folding
  like:%err_r%          general, '_' inside the only middle segment
  like:error%           canonicalised prefix (starts_with)

Each case gets its own plan. A throwaway plan runs first and fills the hot
tier, so every measured plan finds its decompressed chunk images resident and
none of them pays for decompression; the figure is kernel_ns - decomp_ns per
step (def levels + predicate kernels + the count). --runs repeats the whole
case list, cases alternating inside a run, and reports min / median / max per
case. To compare with another build (the parent commit), run that build's
scripts/bench_strpred.py, whose `contains` figure is measured the same way,
alternating with this script. Prints one JSON line."""

import argparse
import json
import os
import shutil
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ["contains:error", "like:%error%", "like:%error%a%",
         "ilike:%error%a%", "like:%err_r%", "like:error%"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cases", nargs="+", default=CASES,
                    help="op:literal, e.g. like:%%error%%a%%")
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
    warm = provider.scan({"select": [{"agg": "count_star"}], "preds": [
        {"col": "message", "op": "contains", "lit": "error"}]})
    warm.execute(0)
    warm.close()
    cases = [tuple(c.split(":", 1)) for c in a.cases]
    ms = {c: [] for c in a.cases}
    info = {}
    for _ in range(a.runs):
        for name, (op, lit) in zip(a.cases, cases):
            q = {"select": [{"agg": "count_star"}],
                 "preds": [{"col": "message", "op": op, "lit": lit}]}
            plan = provider.scan(q)
            plan.load()
            for _ in range(a.warmup):
                plan.execute(0)
            m0 = plan.metrics()
            for _ in range(a.steps):
                batch = plan.execute(0)
            m1 = plan.metrics()
            ms[name].append(((m1["kernel_ns"] - m0["kernel_ns"])
                             - (m1["decomp_ns"] - m0["decomp_ns"]))
                            / a.steps / 1e6)
            info[name] = {
                "cache_hit_frac": round(
                    m1["cache_hit_bytes"] / max(m1["bytes_scanned"], 1), 4),
                "count": batch.column(0).to_pylist()[0],
            }
            plan.close()
    res = {}
    for name in a.cases:
        v = ms[name]
        res[name] = dict(info[name], kernel_ms_per_step={
            "min": round(min(v), 4), "median": round(statistics.median(v), 4),
            "max": round(max(v), 4)})
    if "contains:error" in res:
        base = res["contains:error"]["kernel_ms_per_step"]["median"]
        for name in a.cases:
            res[name]["ratio_to_contains"] = round(
                res[name]["kernel_ms_per_step"]["median"] / base, 4)
    print(json.dumps({"rows": a.rows, "steps": a.steps, "runs": a.runs,
                      "cases": res}))


if __name__ == "__main__":
    main()
