"""count_distinct, host side: the Final merge of its list-state partials
(merge_partials, DistMerger), the staging leg, and plan building under
GPUQ_FAKE_DEVICE (pure host work). Expected values come from
tests/distinct_common.py (plain Python over the data).

Partial layout (include/gpuq.h): keys..., __presence, agg{i}, agg{i}_count —
for a distinct agg both hold the partition-local distinct count — then, after
all fixed columns, one agg{i}_set list column per distinct agg."""

import os
import re

import pyarrow as pa
import pytest
import torch.multiprocessing as mp

from tests import distinct_common as dc
from tests import strpred_common as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

Q_LEVEL = {"select": [{"agg": "count_distinct", "col": "host"}],
           "group_by": ["level"]}


def _partial(keys, presence, sets, typ=pa.string(), key_name="level"):
    """One distinct agg: counts in both slots, the set column last."""
    n = [len(s) for s in sets]
    cols = {}
    if keys is not None:
        cols[key_name] = pa.array(keys, type=pa.string())
    cols["__presence"] = pa.array(presence, type=pa.int64())
    cols["agg0"] = pa.array(n, type=pa.int64())
    cols["agg0_count"] = pa.array(n, type=pa.int64())
    cols["agg0_set"] = pa.array(sets, type=pa.list_(typ))
    return pa.record_batch(cols)


def test_agg_ops_match_header():
    from parseable_amd import _lib

    src = open(os.path.join(ROOT, "include", "gpuq.h")).read()
    end = src.index("} gpuq_agg_op;")
    start = src.rindex("typedef enum {", 0, end) + len("typedef enum {")
    body = re.sub(r"/\*.*?\*/", "", src[start:end], flags=re.S)
    names = [x.partition("=")[0].strip() for x in body.split(",") if x.strip()]
    want = {n[len("GPUQ_AGG_"):].lower(): i for i, n in enumerate(names)}
    assert _lib.AGGS == want
    assert want["count_distinct"] == 5


def test_merge_single_batch_returns_count():
    from parseable_amd.provider import merge_partials

    b = _partial(["INFO", "WARN", None], [5, 2, 1],
                 [["a", "b", "c"], ["a"], []])
    assert merge_partials([b], Q_LEVEL) == [["INFO", 3], ["WARN", 1], [None, 0]]


def test_merge_two_batches_unions():
    from parseable_amd.provider import merge_partials

    b0 = _partial(["INFO", "WARN"], [5, 2], [["a", "b", "c"], ["a"]])
    b1 = _partial(["INFO", "ERROR"], [4, 3], [["b", "c", "d"], ["x", "y"]])
    rows = merge_partials([b0, b1], Q_LEVEL)
    # INFO: |{a,b,c} u {b,c,d}| = 4, not 3 + 3; WARN and ERROR live in one
    # partial only and survive
    assert rows == [["ERROR", 2], ["INFO", 4], ["WARN", 1]]
    assert merge_partials([b1, b0], Q_LEVEL) == rows


def test_merge_numeric_sets():
    from parseable_amd.provider import merge_partials

    q = {"select": [{"agg": "count_distinct", "col": "latency"}],
         "group_by": ["level"]}
    b0 = _partial(["INFO"], [3], [[1, 2, 3]], typ=pa.int64())
    b1 = _partial(["INFO"], [3], [[3, 4, -1]], typ=pa.int64())
    assert merge_partials([b0, b1], q) == [["INFO", 5]]
    b0 = _partial(["INFO"], [3], [[0.5, 0.0, 2.0]], typ=pa.float64())
    b1 = _partial(["INFO"], [3], [[-0.0, 2.0, 7.25]], typ=pa.float64())
    # -0.0 and 0.0 are one value (the f64 key normalisation)
    assert merge_partials([b0, b1], q) == [["INFO", 4]]


def _partial_mixed(keys, presence, sums, sum_cnts, sets, maxs):
    """[count_star, avg latency, count_distinct host, max latency]: the set
    column of agg 2 follows ALL fixed columns."""
    n = [len(s) for s in sets]
    return pa.record_batch({
        "level": pa.array(keys, type=pa.string()),
        "__presence": pa.array(presence, type=pa.int64()),
        "agg0": pa.array(presence, type=pa.int64()),
        "agg0_count": pa.array(presence, type=pa.int64()),
        "agg1": pa.array(sums, type=pa.int64()),
        "agg1_count": pa.array(sum_cnts, type=pa.int64()),
        "agg2": pa.array(n, type=pa.int64()),
        "agg2_count": pa.array(n, type=pa.int64()),
        "agg3": pa.array(maxs, type=pa.int64()),
        "agg3_count": pa.array(sum_cnts, type=pa.int64()),
        "agg2_set": pa.array(sets, type=pa.list_(pa.string())),
    })


Q_MIXED = {"select": [{"agg": "count_star"}, {"agg": "avg", "col": "latency"},
                      {"agg": "count_distinct", "col": "host"},
                      {"agg": "max", "col": "latency"}],
           "group_by": ["level"]}


def test_merge_with_other_aggs():
    from parseable_amd.provider import merge_partials

    b0 = _partial_mixed(["INFO", "WARN"], [4, 2], [40, 6], [4, 2],
                        [["a", "b"], []], [30, 5])
    b1 = _partial_mixed(["INFO", "WARN"], [6, 1], [20, 9], [5, 1],
                        [["b", "c"], ["z"]], [11, 9])
    assert merge_partials([b0], Q_MIXED) == [
        ["INFO", 4, 10.0, 2, 30], ["WARN", 2, 3.0, 0, 5]]
    assert merge_partials([b0, b1], Q_MIXED) == [
        ["INFO", 10, 60 / 9, 3, 30], ["WARN", 3, 5.0, 1, 9]]


def test_merge_no_group_and_empty_rows():
    from parseable_amd.provider import merge_partials

    q = {"select": [{"agg": "count_distinct", "col": "host"}]}
    empty = _partial(None, [0], [[]])       # the empty no-group row
    full = _partial(None, [7], [["a", "b"]])
    assert merge_partials([empty], q) == [[0]]
    assert merge_partials([empty, empty], q) == [[0]]
    assert merge_partials([empty, full], q) == [[2]]
    assert merge_partials([full, full], q) == [[2]]
    assert merge_partials([], q) == [[0]]   # the empty relation: 0, not NULL
    assert merge_partials([None], q) == [[0]]


def test_merge_rejects_partial_without_sets():
    from parseable_amd.provider import GpuqError, merge_partials

    b = _partial(["INFO"], [1], [["a"]])
    b = pa.record_batch([b.column(i) for i in range(b.num_columns - 1)],
                        names=b.schema.names[:-1])
    with pytest.raises(GpuqError, match="agg.*_set"):
        merge_partials([b, b], Q_LEVEL)


def test_dist_merger_world1():
    from parseable_amd.dist import DistMerger

    b = _partial(["INFO", "WARN"], [5, 2], [["a", "b", "c"], []])
    m = DistMerger(Q_LEVEL, device="cpu")
    m.setup(b)
    assert m.step(b) == [["INFO", 3], ["WARN", 0]]
    q = {"select": [{"agg": "count_distinct", "col": "host"}]}
    m = DistMerger(q, device="cpu")
    m.setup(None)
    assert m.step(None) == [[0]]


def _rank_main(rank, world, port, q):
    import torch.distributed as dist

    from parseable_amd.dist import DistMerger

    dist.init_process_group(
        "gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world
    )
    try:
        out = {}
        if rank == 0:
            b = _partial(["INFO", "WARN"], [5, 2], [["a", "b", "c"], ["a"]])
        else:
            b = _partial(["INFO", "ERROR"], [4, 3], [["b", "c", "d"], []])
        m = DistMerger(Q_LEVEL, device="cpu")
        m.setup(b)
        out["overlap"] = m.step(b)

        # one rank without rows: it must still take the set-union path
        nb = _partial(["INFO"], [3], [[1, 2, 3]], typ=pa.int64()) \
            if rank == 0 else None
        qn = {"select": [{"agg": "count_distinct", "col": "latency"}],
              "group_by": ["level"]}
        m = DistMerger(qn, device="cpu")
        m.setup(nb)
        out["one_empty"] = m.step(nb)

        mb = (_partial_mixed(["INFO", "WARN"], [4, 2], [40, 6], [4, 2],
                             [["a", "b"], []], [30, 5]) if rank == 0 else
              _partial_mixed(["INFO", "WARN"], [6, 1], [20, 9], [5, 1],
                             [["b", "c"], ["z"]], [11, 9]))
        m = DistMerger(Q_MIXED, device="cpu")
        m.setup(mb)
        out["mixed"] = m.step(mb)

        # no group, nothing selected on either rank
        q0 = {"select": [{"agg": "count_distinct", "col": "host"}]}
        eb = _partial(None, [0], [[]])
        m = DistMerger(q0, device="cpu")
        m.setup(eb)
        out["empty"] = m.step(eb)
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_dist_merger_gloo_world2():
    import socket

    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(2):
        rank, rows = q.get()
        results[rank] = rows
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for r in (0, 1):
        assert results[r]["overlap"] == [["ERROR", 0], ["INFO", 4], ["WARN", 1]]
        assert results[r]["one_empty"] == [["INFO", 3]]
        assert results[r]["mixed"] == [
            ["INFO", 10, 60 / 9, 3, 30], ["WARN", 3, 5.0, 1, 9]]
        assert results[r]["empty"] == [[0]]


# ---- staging leg -------------------------------------------------------

@pytest.fixture(scope="module")
def staged(tmp_path_factory):
    """Staging .arrows files alone (c6, two files): every row is read by
    StagingScanner on the host."""
    from datagen.gen import gen_staging

    stg = str(tmp_path_factory.mktemp("distinct_staging") / "staging")
    st = gen_staging(stg, config="c6", rows=6_000, n_arrows=2, n_parquet=0,
                     start_minute=10_000)
    data = {}
    for p in st["arrows"]:
        with pa.ipc.open_stream(p) as r:
            t = r.read_all()
        for name in t.column_names:
            c = t.column(name)
            if pa.types.is_string(c.type):
                c = c.cast(pa.binary())
            elif pa.types.is_timestamp(c.type):
                c = c.cast(pa.int64())
            data.setdefault(name, []).extend(c.to_pylist())
    return stg, data


STAGE_QUERIES = [
    {"select": [{"agg": "count_distinct", "col": "level"}]},
    {"select": [{"agg": "count_distinct", "col": "opt_i64"}]},
    {"select": [{"agg": "count_distinct", "col": "p_timestamp"}]},
    {"select": [{"agg": "count_distinct", "col": "tag"}], "group_by": ["level"]},
    {"select": [{"agg": "count_star"}, {"agg": "count_distinct", "col": "sparse"},
                {"agg": "avg", "col": "latency"},
                {"agg": "count_distinct", "col": "level"}],
     "group_by": ["level"],
     "preds": [{"col": "message", "op": "contains", "lit": "rror"}]},
    {"select": [{"agg": "count_distinct", "col": "level"}],
     "preds": [{"col": "message", "op": "contains", "lit": sc.ABSENT}]},
]


@pytest.mark.parametrize("q", STAGE_QUERIES)
def test_staging_aggregate(staged, q):
    from oracle.compare import assert_rows_equal
    from parseable_amd.provider import (StagingScanner, distinct_set_columns,
                                        merge_partials)

    stg, data = staged
    scanner = StagingScanner(stg)
    want = dc.expected(data, q)
    assert_rows_equal(scanner.aggregate(q), want, f"staging {q}")
    b = scanner.partial_batch(q)
    if b is None:
        assert not sc.selected(data, q)
        return
    nk = len(q.get("group_by", []))
    set_cols = distinct_set_columns(q["select"], nk)
    assert b.num_columns == nk + 1 + 2 * len(q["select"]) + len(set_cols)
    for i, ci in set_cols.items():
        sets = b.column(ci)
        assert pa.types.is_list(sets.type) and sets.null_count == 0
        lens = [len(s) for s in sets.to_pylist()]
        assert lens == b.column(nk + 1 + 2 * i).to_pylist()
        assert lens == b.column(nk + 2 + 2 * i).to_pylist()
    # the staging partial merged with itself: a union, the same counts

    def pick(rows):
        return [r[:nk] + [r[nk + i] for i in set_cols] for r in rows]

    assert pick(merge_partials([b, b], q)) == pick(want)


# ---- plan building (GPUQ_FAKE_DEVICE) ----------------------------------

@pytest.fixture(scope="module")
def fake_device():
    os.environ["GPUQ_FAKE_DEVICE"] = "1"
    yield
    os.environ.pop("GPUQ_FAKE_DEVICE", None)


@pytest.fixture(scope="module")
def provider(fake_device, tmp_path_factory):
    from datagen.gen import gen_stream
    from parseable_amd import GpuSession, StandardTableProvider

    td = tmp_path_factory.mktemp("distinct_cpu_c6")
    info = gen_stream(str(td), "s", "c6", **sc.GEN)
    return StandardTableProvider(info["stream_dir"], GpuSession())


def _plan_debug(provider, q, capfd, native=True):
    os.environ["GPUQ_PLAN_DEBUG"] = "1"
    if not native:
        os.environ["GPUQ_PY_PLANNER"] = "1"
    try:
        capfd.readouterr()
        plan = provider.scan(dict(q))
        rows = plan.metrics()["rows_scanned"]
        plan.close()
        return rows, capfd.readouterr().err
    finally:
        os.environ.pop("GPUQ_PLAN_DEBUG", None)
        os.environ.pop("GPUQ_PY_PLANNER", None)


@pytest.mark.parametrize("native", [True, False])
@pytest.mark.parametrize("col,gids", [
    ("level", "dict"), ("tag", "hash"), ("opt_i64", "numeric"),
    ("latency", "numeric"), ("p_timestamp", "numeric"), ("sparse", "dict")])
def test_plan_accepts_op(provider, capfd, native, col, gids):
    q = {"select": [{"agg": "count_distinct", "col": col}]}
    rows, err = _plan_debug(provider, q, capfd, native)
    # a bare count_distinct is a scan, never the manifest count
    assert rows == sc.GEN["rows"]
    assert f"[gpuq plan] distinct agg=0 col={col} gids={gids}" in err, err[-1500:]


def test_plan_fused_paths_off(provider, capfd):
    """The shapes that take fused_count / fused_valagg lose them as soon as a
    distinct agg joins."""
    base_count = {"select": [{"agg": "count_star"}], "group_by": ["level"]}
    base_valagg = {"select": [{"agg": "count_star"},
                              {"agg": "sum", "col": "latency"}],
                   "group_by": ["level"]}
    _, err = _plan_debug(provider, base_count, capfd)
    assert "fused_count=1" in err
    _, err = _plan_debug(provider, base_valagg, capfd)
    assert "fused_valagg=1" in err
    for base in (base_count, base_valagg):
        for col in ("tag", "latency", "level"):
            q = dict(base, select=base["select"]
                     + [{"agg": "count_distinct", "col": col}])
            _, err = _plan_debug(provider, q, capfd)
            assert "[gpuq plan] fused_count=0 fused_valagg=0" in err, err[-1500:]


def _build_error(provider, q):
    from parseable_amd.provider import GpuqError

    with pytest.raises(GpuqError) as ei:
        provider.scan(dict(q))
    return str(ei.value)


def test_plan_build_errors(provider):
    msg = _build_error(provider, {"select": [{"agg": "count_distinct"}]})
    assert "count_distinct needs a column" in msg
    msg = _build_error(provider, {"select": [{"agg": "count_distinct",
                                              "col": "no_such_col"}]})
    assert "no such column: no_such_col" in msg
    msg = _build_error(provider, {
        "select": [{"agg": "count_distinct", "col": "level"}],
        "select_cols": ["p_timestamp", "level"], "limit": 5})
    assert "count_distinct is not allowed in a projection plan" in msg
