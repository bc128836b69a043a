"""Delta fork, plan side (no GPU: plan building is pure host work under
GPUQ_FAKE_DEVICE). The GPUQ_PLAN_DEBUG partition line reports the early
record set: non-zero for a BETWEEN window that cuts a row group, zero for a
window of whole row groups, and for every record kind early + main equals the
count under GPUQ_NO_DELTA_FORK=1. Each plan is built in a subprocess, whose
stderr carries the line."""

import json
import os
import re
import subprocess
import sys

import pytest

from tests.golden_queries import BASE, MIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = """
import json, sys
sys.path.insert(0, sys.argv[1])
from parseable_amd import GpuSession, StandardTableProvider
plan = StandardTableProvider(sys.argv[2], GpuSession()).scan(json.loads(sys.argv[3]))
plan.close()
"""

KINDS = ("segs", "tiles", "tile_recs", "lits_wave", "res")


@pytest.fixture(scope="module")
def stream(tmp_path_factory):
    from datagen.gen import gen_stream

    return gen_stream(str(tmp_path_factory.mktemp("forkcpu")), "fork", "c1",
                      rows=120_000, rows_per_file=40_000, seed=4243)


def plan_counts(stream, lo, hi, serial):
    query = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"}],
             "group_by": ["host"],
             "preds": [{"col": "p_timestamp", "op": "between", "lo": lo, "hi": hi}]}
    env = dict(os.environ, GPUQ_FAKE_DEVICE="1", GPUQ_PLAN_DEBUG="1")
    env.pop("GPUQ_NO_DELTA_FORK", None)
    if serial:
        env["GPUQ_NO_DELTA_FORK"] = "1"
    p = subprocess.run(
        [sys.executable, "-c", SCRIPT, ROOT, stream["stream_dir"], json.dumps(query)],
        env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [ln for ln in p.stderr.splitlines() if "[gpuq plan] part 0:" in ln][-1]
    out = {k: int(v) for k, v in re.findall(r" (\w+)=(\d+)", line)}
    for pre in ("", "early_"):
        a, b = re.search(rf" {pre}res=(\d+)/(\d+)", line).groups()
        out[pre + "res"] = int(a) + int(b)
    return out


def test_cut_window_has_an_early_set(stream):
    lo, hi = BASE + MIN // 3, BASE + 2 * MIN + MIN // 2
    fork = plan_counts(stream, lo, hi, serial=False)
    serial = plan_counts(stream, lo, hi, serial=True)
    assert fork["fork_cols"] == 1 and serial["fork_cols"] == 0
    assert sum(fork["early_" + k] for k in KINDS) > 0, fork
    assert all(serial["early_" + k] == 0 for k in KINDS), serial
    for k in KINDS:
        assert fork[k] + fork["early_" + k] == serial[k], (k, fork, serial)
    assert fork["pages"] == serial["pages"] and fork["chunks"] == serial["chunks"]


def test_whole_row_group_window_has_none(stream):
    lo, hi = BASE + MIN, BASE + 3 * MIN - 1
    fork = plan_counts(stream, lo, hi, serial=False)
    serial = plan_counts(stream, lo, hi, serial=True)
    assert fork["fork_cols"] == 0
    for k in KINDS:
        assert fork["early_" + k] == 0 and fork[k] == serial[k], (k, fork, serial)
