"""LIKE-family (icontains / starts_with / ends_with / not_*) and
is_null / is_not_null predicates, host side: ABI table, plan building through
the native and the Python planner (GPUQ_FAKE_DEVICE — plan building is pure
host work), pruning rules, plan-build errors, and the staging reader.
Expected values come from tests/strpred_common.py (plain Python over the
parquet files)."""

import os
import re

import pytest

from tests import strpred_common as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def fake_device():
    os.environ["GPUQ_FAKE_DEVICE"] = "1"
    yield
    os.environ.pop("GPUQ_FAKE_DEVICE", None)


@pytest.fixture(scope="module")
def c6(tmp_path_factory):
    from datagen.gen import gen_stream

    td = tmp_path_factory.mktemp("strpred_cpu_c6")
    return gen_stream(str(td), "s", "c6", **sc.GEN)


@pytest.fixture(scope="module")
def provider(c6):
    from parseable_amd import GpuSession, StandardTableProvider

    return StandardTableProvider(c6["stream_dir"], GpuSession())


def test_ops_match_header():
    from parseable_amd import _lib

    src = open(os.path.join(ROOT, "include", "gpuq.h")).read()
    body = re.search(r"typedef enum \{(.*?)\} gpuq_op;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    want, nxt = {}, 0
    for item in body.split(","):
        item = item.strip()
        if not item:
            continue
        name, _, val = item.partition("=")
        if val.strip():
            nxt = int(val)
        want[name.strip()[len("GPUQ_"):].lower()] = nxt
        nxt += 1
    assert _lib.OPS == want
    assert want["contains"] == 7 and want["icontains"] == 8
    assert want["is_not_null"] == 16


def _plan_stats(provider, query, native, capfd=None):
    from parseable_amd import EmptyScanResult, ManifestCountResult

    if native:
        os.environ.pop("GPUQ_PY_PLANNER", None)
    else:
        os.environ["GPUQ_PY_PLANNER"] = "1"
    try:
        plan = provider.scan(dict(query))
    finally:
        os.environ.pop("GPUQ_PY_PLANNER", None)
    if isinstance(plan, ManifestCountResult):
        return ("count", plan.count)
    if isinstance(plan, EmptyScanResult):
        return ("empty",)
    try:
        m = plan.metrics()
        return ("scan", m["rows_scanned"], m["bytes_scanned"],
                m["rowgroup_bytes_total"])
    finally:
        plan.close()


COUNT = [{"agg": "count_star"}]


@pytest.mark.parametrize("op", sc.NEW_STR_OPS)
@pytest.mark.parametrize("col,lit", [
    ("message", "error"),
    ("level", "E"),
    # literals outside every file's [min, max] of the column: a min/max
    # comparison would prune, these ops must not
    ("level", "zzzz"), ("level", "!"), ("tag", "zzzz"), ("tag", "!"),
])
def test_string_ops_plan_both_planners_no_pruning(provider, c6, op, col, lit):
    q = {"select": COUNT, "preds": [{"col": col, "op": op, "lit": lit}]}
    a = _plan_stats(provider, q, native=True)
    b = _plan_stats(provider, q, native=False)
    assert a == b, f"native={a} python={b}"
    assert a[0] == "scan" and a[1] == sc.GEN["rows"], a


@pytest.mark.parametrize("op", sc.NULL_OPS)
@pytest.mark.parametrize("col", ["message", "level", "opt_i64", "p_timestamp"])
def test_null_ops_plan_both_planners(provider, op, col):
    q = {"select": COUNT, "preds": [{"col": col, "op": op}]}
    a = _plan_stats(provider, q, native=True)
    b = _plan_stats(provider, q, native=False)
    assert a == b, f"native={a} python={b}"
    if col == "p_timestamp" and op == "is_null":
        assert a == ("empty",)    # never null: every row group dropped
    else:
        assert a[0] == "scan" and a[1] == sc.GEN["rows"], a


@pytest.mark.parametrize("native", [True, False])
def test_required_column_null_ops(provider, native):
    q = {"select": COUNT, "preds": [{"col": "latency", "op": "is_null"}]}
    assert _plan_stats(provider, q, native) == ("empty",)
    q = {"select": COUNT, "preds": [{"col": "latency", "op": "is_not_null"}]}
    a = _plan_stats(provider, q, native)
    assert a[0] == "scan" and a[1] == sc.GEN["rows"]


@pytest.mark.parametrize("native", [True, False])
@pytest.mark.parametrize("op,kept", [("is_null", [1]), ("is_not_null", [0, 2])])
def test_sparse_footer_elision_drops_files(provider, c6, capfd, native, op,
                                           kept):
    """sparse is all-NULL in odd files and null-free in even ones: is_null
    drops exactly the even files, is_not_null exactly the odd ones, and the
    kept ones are proven from the footer (no per-row task)."""
    import pyarrow.parquet as pq

    q = {"select": COUNT, "preds": [{"col": "sparse", "op": op}]}
    os.environ["GPUQ_PLAN_DEBUG"] = "1"
    try:
        capfd.readouterr()
        a = _plan_stats(provider, q, native)
        err = capfd.readouterr().err
    finally:
        os.environ.pop("GPUQ_PLAN_DEBUG", None)
    sizes = [os.path.getsize(f) for f in c6["files"]]
    md = [pq.read_metadata(f) for f in c6["files"]]
    want_rows = sum(md[i].num_rows for i in kept)
    want_rg_bytes = sum(
        md[i].row_group(0).column(c).total_compressed_size
        for i in kept for c in range(md[i].num_columns))
    assert len(sizes) == 3
    assert a[0] == "scan" and a[1] == want_rows and a[3] == want_rg_bytes, a
    m = re.search(r"\[gpuq plan\] pred 0 col=sparse op=%s path=(\S+) rowgroups: "
                  r"nulltask=(\d+) proven=(\d+) pruned=(\d+)" % op, err)
    assert m, err[-2000:]
    assert m.group(1) == "proven+pruned"
    assert [int(m.group(i)) for i in (2, 3, 4)] == [0, len(kept), 3 - len(kept)]


def _build_error(provider, q):
    from parseable_amd.provider import GpuqError

    with pytest.raises(GpuqError) as ei:
        provider.scan(dict(q))
    return str(ei.value)


def test_plan_build_errors(provider):
    msg = _build_error(provider, {"select": COUNT, "preds": [
        {"col": "message", "op": "icontains", "lit": "café"}]})
    assert "icontains literal must be ASCII" in msg
    msg = _build_error(provider, {"select": COUNT, "preds": [
        {"col": "message", "op": "not_icontains", "lit": "État"}]})
    assert "not_icontains literal must be ASCII" in msg
    for op in sc.NEW_STR_OPS:
        msg = _build_error(provider, {"select": COUNT, "preds": [
            {"col": "latency", "op": op, "lit": "1"}]})
        assert f"string predicate {op} on non-utf8 column: latency" in msg
    msg = _build_error(provider, {"select": COUNT, "preds": [
        {"col": "message", "op": "starts_with", "lit": 5}]})
    assert "string column needs string literal: message" in msg
    msg = _build_error(provider, {"select": COUNT, "preds": [
        {"col": "message", "op": "is_null", "lit": "x"}]})
    assert "is_null takes no literal" in msg


def test_like_family_does_not_force_hash_mode(provider, capfd):
    """A LIKE-family predicate alone keeps a column with PLAIN pages on the
    LUT + window paths; an eq predicate next to it moves both to hash."""
    def paths(preds):
        os.environ["GPUQ_PLAN_DEBUG"] = "1"
        try:
            capfd.readouterr()
            plan = provider.scan({"select": COUNT, "preds": preds})
            plan.close()
            err = capfd.readouterr().err
        finally:
            os.environ.pop("GPUQ_PLAN_DEBUG", None)
        return re.findall(r"\[gpuq plan\] pred \d+ col=\S+ op=(\S+) path=(\S+)",
                          err)

    assert paths([{"col": "message", "op": "not_ends_with", "lit": "x"},
                  {"col": "level", "op": "starts_with", "lit": "E"}]) == [
        ("not_ends_with", "lut+window"), ("starts_with", "lut")]
    assert paths([{"col": "message", "op": "icontains", "lit": "x"},
                  {"col": "message", "op": "eq", "lit": "Error"}]) == [
        ("icontains", "hash")]


# ---- staging leg -------------------------------------------------------

STAGE_START = 10_000


@pytest.fixture(scope="module")
def staged(tmp_path_factory):
    """A staging-only stream: an empty manifest list next to a staging
    directory that holds .arrows files alone (n_parquet=0), so every row is
    read by StagingScanner on the host."""
    import json

    import pyarrow as pa

    from datagen.gen import gen_staging

    td = tmp_path_factory.mktemp("strpred_staging")
    sdir = str(td / "s")
    os.makedirs(sdir)
    with open(os.path.join(sdir, "stream.json"), "w") as fh:
        json.dump({"version": "v6", "objectstore-format": "v6",
                   "stream_type": "UserDefined",
                   "snapshot": {"version": "v2", "manifest_list": []}}, fh)
    stg = str(td / "staging")
    st = gen_staging(stg, config="c6", rows=6_000, n_arrows=2, n_parquet=0,
                     start_minute=STAGE_START)
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
    return sdir, stg, st, data


def _staged_rows(staged, q):
    from parseable_amd import Query, StandardTableProvider

    sdir, stg, st, _ = staged
    prov = StandardTableProvider(sdir, None, staging_dir=stg,
                                 now_ms=st["max_ts"])
    rows, _ = Query(prov).execute(dict(q))
    return rows


STAGE_CASES = (
    [("message", op, lit) for op in sc.NEW_STR_OPS
     for lit in ("Error", "error", "TIMEOUT", "r", sc.ABSENT, "")]
    + [("level", op, lit) for op in sc.NEW_STR_OPS
       for lit in sc.level_needles(op)]
    + [(col, op, None) for op in sc.NULL_OPS
       for col in ("message", "level", "opt_i64", "latency")]
)


@pytest.mark.parametrize("col,op,lit", STAGE_CASES)
def test_staging_leg(staged, col, op, lit):
    from oracle.compare import assert_rows_equal

    p = {"col": col, "op": op}
    if lit is not None:
        p["lit"] = lit
    q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"}],
         "group_by": ["level"], "preds": [p]}
    data = staged[3]
    want = sc.expected(data, q)
    assert_rows_equal(_staged_rows(staged, q), want, f"staging {p}")
    n_sel = len(sc.selected(data, q))
    n_nonnull = sum(v is not None for v in data[col])
    all_or_none = lit in (sc.ABSENT, "") or col == "latency"
    if not all_or_none:
        assert 0 < n_sel < n_nonnull or op in sc.NULL_OPS and 0 < n_sel, (
            n_sel, n_nonnull)
