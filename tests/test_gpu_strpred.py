"""LIKE-family (contains / icontains / starts_with / ends_with / not_*) and
is_null / is_not_null predicates on the GPU: the window kernels over PLAIN
pages, the per-dict-entry LUT, k_cmp_str on hash-mode columns, and the
def-level null task. Expected values come from tests/strpred_common.py
(plain Python over the parquet files); the path each predicate took is read
from the GPUQ_PLAN_DEBUG lines
  [gpuq plan] pred <i> col=<c> op=<op> path=lut|window|lut+window|hash|...
  [gpuq plan] part N: ... cwins=<n>

Data: c6, 60,000 rows in three 20,000-row files; each message chunk has dict
pages followed by several PLAIN pages (hundreds of 16 KiB windows)."""

import os
import re

import pytest

from tests import strpred_common as sc

pytestmark = pytest.mark.gpu

BASE, MIN = sc.BASE, sc.MIN
COUNT = [{"agg": "count_star"}]
NEEDLES = ["Error", "error", "TIMEOUT", "r", sc.ABSENT, ""]


@pytest.fixture(scope="module")
def c6(tmp_path_factory):
    from datagen.gen import gen_stream

    td = tmp_path_factory.mktemp("strpred_c6")
    info = gen_stream(str(td), "s", "c6", **sc.GEN)
    info["data"] = sc.load(info["files"])
    return info


@pytest.fixture(scope="module")
def session():
    from parseable_amd import GpuSession

    return GpuSession()


def _gpu(info, session, q, capfd):
    """-> (rows, [(pred index, col, op, path)], plan debug text)"""
    from parseable_amd import Query, StandardTableProvider

    os.environ["GPUQ_PLAN_DEBUG"] = "1"
    try:
        capfd.readouterr()
        prov = StandardTableProvider(info["stream_dir"], session)
        rows, _ = Query(prov).execute(dict(q))
        err = capfd.readouterr().err
    finally:
        os.environ.pop("GPUQ_PLAN_DEBUG", None)
    paths = re.findall(
        r"\[gpuq plan\] pred (\d+) col=(\S+) op=(\S+) path=(\S+)", err)
    return rows, paths, err


def _check(info, session, q, capfd, vacuous_ok=False):
    """Run q, compare with the Python expected rows, and (unless the case is
    declared all-or-none) require 0 < selected < non-null rows of the first
    predicate's column."""
    from oracle.compare import assert_rows_equal

    data = info["data"]
    rows, paths, err = _gpu(info, session, q, capfd)
    assert_rows_equal(rows, sc.expected(data, q), f"GPU vs python: {q}")
    if not vacuous_ok:
        in_range = sc.selected(data, {"time_range": q.get("time_range")})
        col = data[q["preds"][0]["col"]]
        non_null = sum(col[i] is not None for i in in_range)
        if q["preds"][0]["op"] in sc.NULL_OPS:
            non_null = len(in_range)   # a null op: some, not all, rows
        n_sel = len(sc.selected(data, q))
        assert 0 < n_sel < non_null, (q, n_sel, non_null)
    return rows, paths, err


def _pred(col, op, lit=None):
    p = {"col": col, "op": op}
    if lit is not None:
        p["lit"] = lit
    return p


@pytest.mark.parametrize("op", sc.STR_OPS)
def test_window_and_lut(c6, session, capfd, op):
    for lit in NEEDLES:
        q = {"select": COUNT, "preds": [_pred("message", op, lit)]}
        rows, paths, err = _check(c6, session, q, capfd,
                                  vacuous_ok=lit in (sc.ABSENT, ""))
        assert paths == [("0", "message", op, "lut+window")], paths
        m = re.search(r"\[gpuq plan\] part 0: .* cwins=(\d+)", err)
        assert m and int(m.group(1)) > 0, err[-1500:]
        n_nonnull = sum(v is not None for v in c6["data"]["message"])
        if lit in (sc.ABSENT, ""):
            all_rows = (lit == "") != op.startswith("not_")
            assert rows == [[n_nonnull if all_rows else 0]], (op, lit, rows)


@pytest.mark.parametrize("op", sc.STR_OPS)
def test_lut_only(c6, session, capfd, op):
    for lit in sc.level_needles(op):
        q = {"select": [{"agg": "count_star"},
                        {"agg": "max", "col": "latency"}],
             "group_by": ["level"], "preds": [_pred("level", op, lit)]}
        _, paths, _ = _check(c6, session, q, capfd)
        assert paths == [("0", "level", op, "lut")], paths


@pytest.mark.parametrize("op,lit", [
    ("contains", "ag-0001"), ("icontains", "TAG-0002"),
    ("starts_with", "Tag-"), ("ends_with", "7"),
    ("not_contains", "ag-0001"), ("not_icontains", "TAG-0002"),
    ("not_starts_with", "Tag-"), ("not_ends_with", "7"),
])
def test_hash_mode(c6, session, capfd, op, lit):
    q = {"select": COUNT, "group_by": ["tag"], "preds": [_pred("tag", op, lit)]}
    _, paths, _ = _check(c6, session, q, capfd)
    assert paths == [("0", "tag", op, "hash")], paths


def test_conjunctions(c6, session, capfd):
    q = {"select": COUNT,
         "preds": [_pred("message", "contains", "rror"),
                   _pred("message", "not_contains", "TIMEOUT")],
         "time_range": [BASE + MIN + 5_000, BASE + MIN + 45_000]}
    _, paths, _ = _check(c6, session, q, capfd)
    assert [p[3] for p in paths] == ["lut+window", "lut+window"]
    q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"}],
         "group_by": ["level"],
         "preds": [_pred("message", "icontains", "error"),
                   _pred("level", "not_starts_with", "E")]}
    _, paths, _ = _check(c6, session, q, capfd)
    assert [p[3] for p in paths] == ["lut+window", "lut"]


def test_projection(c6, session, capfd):
    """Top-50 projection under ends_with. p_timestamp repeats within a file,
    and rows of equal timestamp have no defined order: the timestamp
    sequence must be equal as is, the rows after ordering ties."""
    q = {"select_cols": ["p_timestamp", "level", "latency"], "limit": 50,
         "preds": [_pred("message", "ends_with", "error")]}
    data = c6["data"]
    rows, paths, _ = _gpu(c6, session, q, capfd)
    assert paths == [("0", "message", "ends_with", "lut+window")]
    want_all = sc.expected(data, dict(q, limit=None))
    assert 50 < len(want_all) < sum(v is not None for v in data["message"])
    # no tie across the cut, so the top-50 row set is unique
    assert want_all[49][0] != want_all[50][0]
    want = want_all[:50]
    assert [r[0] for r in rows] == [r[0] for r in want]
    canon = lambda rs: sorted(rs, key=lambda r: (-r[0], str(r[1]), r[2]))
    assert canon(rows) == canon(want)


def test_oversized_value(c6, session, capfd):
    """File 0 holds one 40,000-byte message (Error ... TIMEOUT): larger than
    a window, it takes the single-value branch of every window kernel."""
    data = c6["data"]
    big = [i for i, v in enumerate(data["message"])
           if v is not None and len(v) > 16384]
    assert len(big) == 1 and data["__file"][big[0]] == 0
    assert len(data["message"][big[0]]) == 40_000
    tr = [BASE, BASE + MIN]
    for preds in (
        [_pred("message", "starts_with", "Error"),
         _pred("message", "ends_with", "TIMEOUT")],
        [_pred("message", "contains", "TIMEOUT")],
        [_pred("message", "not_contains", "TIMEOUT")],
        [_pred("message", "icontains", "timeout")],
        [_pred("message", "not_icontains", "TIMEOUT")],
        [_pred("message", "not_starts_with", "Error")],
        [_pred("message", "not_ends_with", "TIMEOUT")],
    ):
        q = {"select": COUNT, "preds": preds, "time_range": tr}
        neg = preds[0]["op"].startswith("not_")
        assert (big[0] in sc.selected(data, q)) == (not neg)
        _check(c6, session, q, capfd)
    # the big row alone: everything else that starts with Error and ends
    # with TIMEOUT is excluded by length-independent means
    q = {"select": [{"agg": "count_star"}, {"agg": "min", "col": "latency"}],
         "preds": [_pred("message", "starts_with", "Error "),
                   _pred("message", "ends_with", "xTIMEOUT")],
         "time_range": tr}
    assert sc.selected(data, q) == big
    _check(c6, session, q, capfd)


@pytest.mark.parametrize(
    "op", ["contains", "icontains", "not_contains", "not_icontains"])
def test_queue_overflow(c6, session, capfd, op):
    """File 1 holds a run of messages that are nearly all '=': a window
    inside it has far more than the 4,096 candidate positions the substring
    kernel queues for a needle starting with '=', so the kernel drops the
    queue and sweeps the staged window."""
    data = c6["data"]
    msg = data["message"]
    run = [i for i, v in enumerate(msg)
           if v is not None and v.startswith(b"=" * 120)]
    # contiguous, >= three windows of [u32 len][bytes] records, >= 90 % '=':
    # whatever the window and page alignment, some window lies inside the
    # run and holds > 0.9 * (16384 - one record) candidates
    assert run == list(range(run[0], run[0] + len(run)))
    assert {data["__file"][i] for i in run} == {1}
    n_bytes = sum(4 + len(msg[i]) for i in run)
    assert n_bytes >= 3 * 16384
    assert sum(msg[i].count(b"=") for i in run) >= 0.9 * n_bytes
    for lit in ("=Error", "=error", "==", "=x"):
        q = {"select": COUNT, "preds": [_pred("message", op, lit)],
             "time_range": [BASE + MIN, BASE + 2 * MIN]}
        _, paths, _ = _check(c6, session, q, capfd)
        assert paths == [("0", "message", op, "lut+window")], paths


@pytest.mark.parametrize("op", sc.NULL_OPS)
@pytest.mark.parametrize("col", ["message", "level", "opt_i64", "tag"])
def test_null_predicates(c6, session, capfd, op, col):
    data = c6["data"]
    q = {"select": COUNT, "preds": [_pred(col, op)]}
    rows, paths, _ = _gpu(c6, session, q, capfd)
    n_null = sum(v is None for v in data[col])
    assert 0 < n_null < len(data[col])
    assert rows == [[n_null if op == "is_null" else len(data[col]) - n_null]]
    assert paths == [("0", col, op, "nulltask")], paths


@pytest.mark.parametrize("op,kept", [("is_null", [1]), ("is_not_null", [0, 2])])
def test_null_predicates_sparse(c6, session, capfd, op, kept):
    data = c6["data"]
    q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"}],
         "group_by": ["level"], "preds": [_pred("sparse", op)]}
    rows, paths, err = _gpu(c6, session, q, capfd)
    from oracle.compare import assert_rows_equal

    assert_rows_equal(rows, sc.expected(data, q), str(q))
    assert {data["__file"][i] for i in sc.selected(data, q)} == set(kept)
    assert paths == [("0", "sparse", op, "proven+pruned")], paths
    m = re.search(r"nulltask=(\d+) proven=(\d+) pruned=(\d+)", err)
    assert [int(g) for g in m.groups()] == [0, len(kept), 3 - len(kept)]


def test_null_predicates_required_column(c6, session, capfd):
    """latency is a required column: is_not_null is a no-op, is_null selects
    nothing."""
    data = c6["data"]
    q = {"select": [{"agg": "count_star"}, {"agg": "sum", "col": "latency"}],
         "preds": [_pred("latency", "is_not_null")]}
    rows, paths, _ = _gpu(c6, session, q, capfd)
    assert rows == [[len(data["latency"]), sum(data["latency"])]]
    assert paths == [("0", "latency", "is_not_null", "proven")]
    q = {"select": COUNT, "group_by": ["level"],
         "preds": [_pred("latency", "is_null")]}
    rows, _, _ = _gpu(c6, session, q, capfd)
    assert rows == []
    q = {"select": COUNT, "preds": [_pred("latency", "is_null")]}
    rows, _, _ = _gpu(c6, session, q, capfd)
    assert rows == [[0]]


def test_null_predicate_conjunctions(c6, session, capfd):
    q = {"select": COUNT,
         "preds": [_pred("message", "is_not_null"),
                   _pred("message", "not_icontains", "error")]}
    _, paths, _ = _check(c6, session, q, capfd)
    assert [p[3] for p in paths] == ["nulltask", "lut+window"]
    q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"}],
         "group_by": ["level"], "preds": [_pred("opt_i64", "is_null")]}
    _check(c6, session, q, capfd)
    q = {"select": [{"agg": "count_star"}, {"agg": "sum", "col": "opt_i64"}],
         "group_by": ["level"],
         "preds": [_pred("opt_i64", "is_not_null"),
                   _pred("message", "is_null")]}
    _check(c6, session, q, capfd)


def test_same_query_twice_hot_tier(c6, capfd):
    """Second run in one session: the decompressed chunk images come from
    the hot tier; the answer must not change."""
    from parseable_amd import GpuSession, Query, StandardTableProvider

    sess = GpuSession()
    q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"}],
         "group_by": ["level"],
         "preds": [_pred("message", "icontains", "TimeOut")]}
    prov = StandardTableProvider(c6["stream_dir"], sess)
    rows1, m1 = Query(prov).execute(dict(q))
    rows2, m2 = Query(prov).execute(dict(q))
    assert rows1 == rows2 == sc.expected(c6["data"], q)
    assert m1["cache_hit_bytes"] == 0 and m2["cache_hit_bytes"] > 0
    assert 0 < len(sc.selected(c6["data"], q)) < 60_000
