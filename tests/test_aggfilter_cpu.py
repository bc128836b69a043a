"""Per-aggregate FILTER (`{"agg": ..., "filter": ...}` in query["select"]),
host side: the gpuq_agg_filter ABI and its validation, the pred order of
_build_c_query, both planners (filters never prune, never bound the time
window, never take the count fast path — GPUQ_FAKE_DEVICE, plan building is
pure host work), the staging reader, merge_partials, a world-2 gloo
DistMerger run, and the plain-Python reference of tests/aggfilter_common.py
itself."""

import ctypes as C
import os
import re

import pyarrow as pa
import pytest
import torch.multiprocessing as mp

from tests import aggfilter_common as ac
from tests import where_common as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE, MIN = wc.BASE, wc.MIN
L = wc.leaf
LEAF, AND, OR = 0, 1, 2
ROWS = wc.GEN["rows_per_file"]

ERR = L("level", "eq", "ERROR")
NOPE = L("level", "eq", "NOPE")
SLOW = L("latency", "ge", 900_000)
TMO = L("message", "icontains", "timeout")


def in_file(i):
    return {"col": "p_timestamp", "op": "between", "lo": BASE + i * MIN,
            "hi": BASE + (i + 1) * MIN - 1}


@pytest.fixture(scope="module", autouse=True)
def fake_device():
    os.environ["GPUQ_FAKE_DEVICE"] = "1"
    yield
    os.environ.pop("GPUQ_FAKE_DEVICE", None)


@pytest.fixture(scope="module")
def c6(tmp_path_factory):
    from datagen.gen import gen_stream

    td = tmp_path_factory.mktemp("aggfilter_cpu_c6")
    info = gen_stream(str(td), "s", "c6", **wc.GEN)
    info["data"] = wc.load(info["files"])
    return info


@pytest.fixture(scope="module")
def provider(c6):
    from parseable_amd import GpuSession, StandardTableProvider

    return StandardTableProvider(c6["stream_dir"], GpuSession())


# ---- the reference ------------------------------------------------------------

def cpu_queries():
    """The filtered queries of this module, every aggregate kind among them."""
    f_or = {"or": [ERR, {"and": [SLOW, TMO]}]}
    return [
        {"select": [{"agg": "count_star"}, {"agg": "count_star", "filter": SLOW}],
         "group_by": ["level"]},
        {"select": [{"agg": "count_star", "filter": NOPE},
                    {"agg": "max", "col": "latency", "filter": NOPE},
                    {"agg": "count_distinct", "col": "sparse", "filter": NOPE}],
         "group_by": ["level"]},
        {"select": [{"agg": "count_star", "filter": NOPE},
                    {"agg": "sum", "col": "f_f64", "filter": NOPE}]},
        {"select": [{"agg": "count", "col": "opt_i64", "filter": f_or},
                    {"agg": "sum", "col": "opt_i64", "filter": SLOW},
                    {"agg": "sum", "col": "f_f64", "filter": TMO},
                    {"agg": "avg", "col": "latency", "filter": ERR},
                    {"agg": "min", "col": "f_f64", "filter": f_or},
                    {"agg": "max", "col": "message", "filter": SLOW},
                    {"agg": "count_distinct", "col": "tag", "filter": ERR},
                    {"agg": "max", "col": "latency"}],
         "group_by": ["level"], "preds": [L("latency", "ne", 7)],
         "where": {"or": [L("f_f64", "lt", 0.5), L("opt_i64", "is_null")]}},
        {"select": [{"agg": "count_star", "filter": ERR}],
         "preds": [L("level", "ne", "ERROR")]},
        {"select": [{"agg": "min", "col": "latency", "filter": in_file(1)}],
         "time_range": [BASE, BASE + 2 * MIN], "group_by": ["level"]},
    ]


@pytest.mark.parametrize("qi", range(6))
def test_reference_cross_check(c6, qi):
    q = cpu_queries()[qi]
    ac.cross_check(c6["data"], q)


def test_reference_keeps_groups_of_where(c6):
    data = c6["data"]
    rows = ac.expected(data, cpu_queries()[1])
    plain = wc.expected(data, {"select": [{"agg": "count_star"}],
                               "group_by": ["level"]})
    assert [r[0] for r in rows] == [r[0] for r in plain] and len(rows) > 1
    assert all(r[1:] == [0, None, 0] for r in rows)
    assert ac.expected(data, cpu_queries()[2]) == [[0, None]]


# ---- ABI --------------------------------------------------------------------------

def test_lib_matches_header():
    from parseable_amd import _lib

    src = open(os.path.join(ROOT, "include", "gpuq.h")).read()
    m = re.search(r"typedef struct \{([^}]*)\} gpuq_agg_filter;", src)
    fields = [re.sub(r"/\*.*?\*/", "", f, flags=re.S).split()[-1].lstrip("*")
              for f in m.group(1).split(";") if f.strip() and
              re.sub(r"/\*.*?\*/", "", f, flags=re.S).strip()]
    assert fields == [n for n, _ in _lib.GpuqAggFilter._fields_]
    assert C.sizeof(_lib.GpuqAggFilter) == 24
    lib = _lib.load()
    for base in ("gpuq_plan_build", "gpuq_plan_build_from_stream"):
        decl = re.search(r"gpuq_plan\* %s_filtered\((.*?)\);" % base, src, re.S)
        assert decl and decl.group(1).rstrip().endswith(
            "const gpuq_agg_filter* filters, int32_t n_filters")
        old, new = getattr(lib, base + "_where"), getattr(lib, base + "_filtered")
        assert new.argtypes[:-2] == old.argtypes
        assert new.argtypes[-1] is C.c_int32


def _raw_build(provider, c6, preds, nodes, filters, native, select=None,
               select_cols=None):
    """Build a plan from raw arrays: `nodes` the WHERE node list
    [(kind, parent, pred)], `filters` [(agg, node list)]. -> None when the plan
    builds, else the library's error text."""
    from parseable_amd import _lib
    from parseable_amd.provider import _build_c_projection, _build_c_query

    lib = _lib.load()
    sess = provider.session
    keep = []
    q = {"select": select or [{"agg": "count_star"},
                              {"agg": "max", "col": "latency"}],
         "preds": preds}
    if select_cols:
        q["select_cols"] = select_cols
    cpreds, np_, cgroup, ng, caggs, na = _build_c_query(q, keep)
    cproj, nproj, limit = _build_c_projection(q, keep)

    def c_nodes(nodes):
        cn = (_lib.GpuqWhereNode * max(len(nodes), 1))()
        for i, (k, par, pr) in enumerate(nodes):
            cn[i].kind, cn[i].parent, cn[i].pred = k, par, pr
        keep.append(cn)
        return cn

    cn = c_nodes(nodes)
    cf = (_lib.GpuqAggFilter * max(len(filters), 1))()
    for j, (agg, fnodes) in enumerate(filters):
        cf[j].agg, cf[j].nodes, cf[j].n_nodes = agg, c_nodes(fnodes), len(fnodes)
    if native:
        fc = C.c_int64(-1)
        plan = lib.gpuq_plan_build_from_stream_filtered(
            sess._ctx, c6["stream_dir"].encode(), cproj, nproj, cpreds, np_,
            cgroup, ng, caggs, na, C.c_int64(limit), C.byref(fc), cn,
            len(nodes), cf, len(filters))
        if not plan and fc.value != -1:
            return None
    else:
        files = (_lib.GpuqFile * len(c6["files"]))()
        pb = [p.encode() for p in c6["files"]]
        for i, b in enumerate(pb):
            files[i].path, files[i].row_groups, files[i].n_row_groups = b, None, -1
        plan = lib.gpuq_plan_build_filtered(
            sess._ctx, files, len(pb), cproj, nproj, cpreds, np_, cgroup, ng,
            caggs, na, C.c_int64(limit), cn, len(nodes), cf, len(filters))
    if plan:
        lib.gpuq_plan_destroy(plan)
        return None
    return sess._err()


P3 = [ERR, L("latency", "lt", 1000), L("opt_i64", "gt", 5)]
ONE = lambda p: [(LEAF, -1, p)]  # noqa: E731


def _or_chain(n_or, first_pred):
    """OR(leaf, AND(leaf, OR(...))) with n_or OR levels -> (preds, nodes)"""
    nodes, preds, parent = [], [], -1
    for d in range(n_or):
        nodes.append((OR, parent, -1))
        o = len(nodes) - 1
        nodes.append((LEAF, o, first_pred + len(preds)))
        preds.append(L("latency", "lt", 1000 + d))
        nodes.append((AND, o, -1))
        a = len(nodes) - 1
        nodes.append((LEAF, a, first_pred + len(preds)))
        preds.append(L("opt_i64", "gt", d))
        parent = a
    nodes.append((LEAF, parent, first_pred + len(preds)))
    preds.append(ERR)
    return preds, nodes


BAD = [
    ("agg out of range", P3[:2], [(LEAF, -1, 0)], [(2, ONE(1))],
     "agg index out of range"),
    ("negative agg", P3[:2], [(LEAF, -1, 0)], [(-1, ONE(1))],
     "agg index out of range"),
    ("two filters on one agg", P3, [(LEAF, -1, 0)], [(1, ONE(1)), (1, ONE(2))],
     "already has a filter"),
    ("pred shared with where", P3[:2], [(AND, -1, -1), (LEAF, 0, 0), (LEAF, 0, 1)],
     [(0, ONE(1))], "more than one leaf"),
    ("pred shared by two filters", P3[:2], [(LEAF, -1, 0)],
     [(0, ONE(1)), (1, ONE(1))], "more than one leaf"),
    ("unused pred", P3, [(LEAF, -1, 0)], [(0, ONE(1))], "used by no leaf"),
    ("childless group", P3[:2], [(LEAF, -1, 0)],
     [(0, [(AND, -1, -1), (LEAF, 0, 1), (OR, 0, -1)])],
     "at least one condition or group"),
    ("empty filter tree", P3[:1], [(LEAF, -1, 0)], [(0, [])],
     "at least one node"),
    ("filter root parent", P3[:2], [(LEAF, -1, 0)], [(0, [(LEAF, 0, 1)])],
     "parent must be -1"),
    ("filter pred out of range", P3[:2], [(AND, -1, -1), (LEAF, 0, 0), (LEAF, 0, 1)],
     [(0, ONE(2))], "names no predicate"),
]


@pytest.mark.parametrize("native", [True, False])
@pytest.mark.parametrize("name,preds,nodes,filters,msg", BAD,
                         ids=[b[0] for b in BAD])
def test_validation_errors(provider, c6, native, name, preds, nodes, filters,
                           msg):
    err = _raw_build(provider, c6, preds, nodes, filters, native)
    assert err is not None and msg in err, err


@pytest.mark.parametrize("native", [True, False])
def test_limits(provider, c6, native):
    # 32 leaves over WHERE and all filters together
    preds = [L("latency", "ne", i) for i in range(33)]
    where = [(AND, -1, -1)] + [(LEAF, 0, i) for i in range(20)]

    def filt(lo, hi):
        return [(OR, -1, -1)] + [(LEAF, 0, i) for i in range(lo, hi)]

    err = _raw_build(provider, c6, preds, where, [(0, filt(20, 33))], native)
    assert err and "more than 32 leaves" in err, err
    assert _raw_build(provider, c6, preds[:32], where, [(0, filt(20, 32))],
                      native) is None
    # ... also when WHERE is the implied AND of the preds no filter uses
    err = _raw_build(provider, c6, preds, [], [(0, filt(20, 33))], native)
    assert err and "more than 32 leaves" in err, err
    assert _raw_build(provider, c6, preds[:32], [], [(0, filt(20, 32))],
                      native) is None
    # OR depth: 5 inside a filter fails, 4 builds — per tree, next to a WHERE
    # tree of depth 4
    wp, wn = _or_chain(4, 0)
    fp, fn = _or_chain(5, len(wp))
    err = _raw_build(provider, c6, wp + fp, wn, [(1, fn)], native)
    assert err and "OR nesting depth above 4" in err, err
    fp, fn = _or_chain(4, len(wp))
    assert _raw_build(provider, c6, wp + fp, wn, [(1, fn)], native) is None
    # at most MAX_AGGS filters: a ninth has no aggregate to sit on
    sel = [{"agg": "count_star"}] * 8
    p9 = [L("latency", "ne", i) for i in range(9)]
    assert _raw_build(provider, c6, p9[:8], [],
                      [(i, ONE(i)) for i in range(8)], native, select=sel) is None
    err = _raw_build(provider, c6, p9, [],
                     [(i, ONE(i)) for i in range(8)] + [(7, ONE(8))], native,
                     select=sel)
    assert err and "already has a filter" in err, err


@pytest.mark.parametrize("native", [True, False])
def test_filter_with_projection_is_an_error(provider, c6, native):
    err = _raw_build(provider, c6, P3[:1], [], [(0, ONE(0))], native,
                     select_cols=["p_timestamp", "level"])
    assert err and "not allowed in a projection plan" in err, err


def test_python_surface_errors(provider):
    from parseable_amd.provider import GpuqError

    with pytest.raises(GpuqError, match="at least one condition or group"):
        provider.scan({"select": [{"agg": "count_star",
                                   "filter": {"or": [ERR, {"and": []}]}}]})
    with pytest.raises(GpuqError, match="exactly one key"):
        provider.scan({"select": [{"agg": "count_star",
                                   "filter": {"and": [ERR], "or": [SLOW]}}]})


# ---- pred order ---------------------------------------------------------------------

def test_pred_order_and_structs():
    from parseable_amd import _lib
    from parseable_amd.provider import (_build_c_filters, _build_c_query,
                                        _build_c_where)

    f1 = {"or": [ERR, {"and": [SLOW, TMO]}]}
    q = {"select": [{"agg": "count_star"},
                    {"agg": "max", "col": "latency", "filter": f1},
                    {"agg": "count_star", "filter": NOPE}],
         "preds": [L("latency", "ne", 7)],
         "time_range": [BASE, BASE + MIN],
         "where": {"or": [L("f_f64", "lt", 0.5), L("opt_i64", "is_null")]}}
    keep = []
    cpreds, np_, _, _, caggs, na = _build_c_query(q, keep)
    got = [(cpreds[i].column.decode(), cpreds[i].op) for i in range(np_)]
    assert got == [("latency", _lib.OPS["ne"]), ("p_timestamp", _lib.OPS["between"]),
                   ("f_f64", _lib.OPS["lt"]), ("opt_i64", _lib.OPS["is_null"]),
                   ("level", _lib.OPS["eq"]), ("latency", _lib.OPS["ge"]),
                   ("message", _lib.OPS["icontains"]), ("level", _lib.OPS["eq"])]
    assert cpreds[7].str == b"NOPE" and na == 3
    cn, nn = _build_c_where(q, keep)
    assert [(cn[i].kind, cn[i].parent, cn[i].pred) for i in range(nn)] == [
        (AND, -1, -1), (LEAF, 0, 0), (LEAF, 0, 1), (OR, 0, -1), (LEAF, 3, 2),
        (LEAF, 3, 3)]
    cf, nf = _build_c_filters(q, keep)
    assert nf == 2 and (cf[0].agg, cf[0].n_nodes) == (1, 5)
    assert [(cf[0].nodes[i].kind, cf[0].nodes[i].parent, cf[0].nodes[i].pred)
            for i in range(5)] == [(OR, -1, -1), (LEAF, 0, 4), (AND, 0, -1),
                                   (LEAF, 2, 5), (LEAF, 2, 6)]
    assert (cf[1].agg, cf[1].n_nodes) == (2, 1)
    assert (cf[1].nodes[0].kind, cf[1].nodes[0].parent,
            cf[1].nodes[0].pred) == (LEAF, -1, 7)
    # flat WHERE + filters: no WHERE node list, WHERE is the AND of the rest
    q2 = {"select": [{"agg": "count_star", "filter": ERR}], "preds": [SLOW]}
    assert _build_c_where(q2, keep) == (None, 0)
    cf, nf = _build_c_filters(q2, keep)
    assert nf == 1 and cf[0].nodes[0].pred == 1
    assert _build_c_filters({"select": [{"agg": "count_star"}]}, keep) == (None, 0)


# ---- both planners --------------------------------------------------------------------

def _scan(provider, query, native, capfd=None):
    """-> (kind, rows_scanned or count, plan-debug text)"""
    from parseable_amd import EmptyScanResult, ManifestCountResult

    os.environ.pop("GPUQ_PY_PLANNER", None)
    if not native:
        os.environ["GPUQ_PY_PLANNER"] = "1"
    if capfd is not None:
        os.environ["GPUQ_PLAN_DEBUG"] = "1"
        capfd.readouterr()
    try:
        plan = provider.scan(dict(query))
    finally:
        os.environ.pop("GPUQ_PY_PLANNER", None)
        os.environ.pop("GPUQ_PLAN_DEBUG", None)
    err = capfd.readouterr().err if capfd is not None else ""
    if isinstance(plan, ManifestCountResult):
        return "count", plan.count, err
    if isinstance(plan, EmptyScanResult):
        return "empty", 0, err
    try:
        return "scan", plan.metrics()["rows_scanned"], err
    finally:
        plan.close()


@pytest.mark.parametrize("native", [True, False])
def test_filter_leaves_never_prune(provider, capfd, native):
    # as WHERE each of these drops files (or all of them) by min/max or footer
    # null counts; as a filter none does
    for f in (L("latency", "lt", -5), in_file(0), L("latency", "is_null"),
              {"or": [in_file(0), in_file(2)]},
              {"and": [L("p_timestamp", "lt", BASE - 5), ERR]}):
        as_where = _scan(provider, {"select": [{"agg": "count_star"}],
                                    "group_by": ["level"], "where": f}, native)
        assert as_where[:2] != ("scan", 3 * ROWS), f
        a = _scan(provider, {"select": [{"agg": "count_star", "filter": f}],
                             "group_by": ["level"]}, native, capfd)
        assert a[:2] == ("scan", 3 * ROWS), (f, a[:2])
        assert re.search(r"\[gpuq plan\] agg 0 filter \S.* ctx=1", a[2]), a[2][-1500:]


@pytest.mark.parametrize("native", [True, False])
def test_timestamp_filter_leaf_does_not_narrow_the_window(provider, native):
    tr = [BASE, BASE + 2 * MIN]
    q = {"select": [{"agg": "count_star"},
                    {"agg": "count_star", "filter": in_file(0)}],
         "group_by": ["level"], "time_range": tr}
    assert _scan(provider, q, native)[:2] == ("scan", 2 * ROWS)
    q = {"select": [{"agg": "count_star", "filter": L("p_timestamp", "lt", BASE)}],
         "group_by": ["level"]}
    assert _scan(provider, q, native)[:2] == ("scan", 3 * ROWS)


@pytest.mark.parametrize("native", [True, False])
def test_bare_filtered_count_is_not_a_manifest_count(provider, native):
    tr = [BASE, BASE + MIN]
    assert _scan(provider, {"select": [{"agg": "count_star"}], "time_range": tr},
                 native)[:2] == ("count", ROWS)
    for f in (ERR, in_file(0)):
        q = {"select": [{"agg": "count_star", "filter": f}]}
        assert _scan(provider, q, native)[:2] == ("scan", 3 * ROWS), f
        assert _scan(provider, dict(q, time_range=tr), native)[:2] == (
            "scan", ROWS), f


@pytest.mark.parametrize("native", [True, False])
def test_unfiltered_plans_are_unchanged(provider, capfd, native):
    """A plan without filters prints no filter line and no tree for a flat
    WHERE; one with filters keeps off both fused paths."""
    q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"}],
         "group_by": ["level"], "preds": [SLOW]}
    a = _scan(provider, q, native, capfd)
    assert "filter" not in a[2] and "[gpuq plan] where" not in a[2]
    q = {"select": [{"agg": "count_star"}], "group_by": ["level"]}
    assert "fused_count=1" in _scan(provider, q, native, capfd)[2]
    q = {"select": [{"agg": "count_star"},
                    {"agg": "count_star", "filter": ERR}], "group_by": ["level"]}
    b = _scan(provider, q, native, capfd)
    assert "fused_count=0 fused_valagg=0" in b[2]
    assert re.search(r"\[gpuq plan\] where pred 0 col=level op=eq ctx=1 ", b[2])


@pytest.mark.parametrize("native", [True, False])
def test_filter_or_over_one_column_folds_into_its_lut(provider, capfd, native):
    f = {"or": [ERR, L("level", "eq", "warn")]}
    a = _scan(provider, {"select": [{"agg": "count_star", "filter": f}],
                         "group_by": ["level"]}, native, capfd)
    assert re.findall(r"\[gpuq plan\] or node=\d+ terms=2 path=(\w+)", a[2]) == [
        "lut"], a[2][-1500:]


# ---- staging ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def staged(tmp_path_factory):
    import json

    from datagen.gen import gen_staging

    td = tmp_path_factory.mktemp("aggfilter_staging")
    sdir = str(td / "s")
    os.makedirs(sdir)
    with open(os.path.join(sdir, "stream.json"), "w") as fh:
        json.dump({"version": "v6", "objectstore-format": "v6",
                   "stream_type": "UserDefined",
                   "snapshot": {"version": "v2", "manifest_list": []}}, fh)
    stg = str(td / "staging")
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
    return sdir, stg, st, data


@pytest.mark.parametrize("qi", range(5))
def test_staging_leg(staged, qi):
    from oracle.compare import FLOAT_RTOL, assert_rows_equal, rows_equal
    from parseable_amd import Query, StandardTableProvider

    sdir, stg, st, data = staged
    prov = StandardTableProvider(sdir, None, staging_dir=stg, now_ms=st["max_ts"])
    q = cpu_queries()[qi]
    rows, _ = Query(prov).execute(dict(q))
    want = ac.expected(data, q)
    # the staging leg adds f64 sums in row order (an order-dependent engine in
    # oracle.compare's terms); everything but floats compares exactly
    assert_rows_equal(rows, want, f"staging {q}", float_rtol=FLOAT_RTOL)
    # the filters matter: the unfiltered answer differs
    assert not rows_equal(want, ac.expected(data, ac.strip(q)))


# ---- merges ------------------------------------------------------------------------------

MQ = {"select": [{"agg": "count_star"},
                 {"agg": "count_star", "filter": ERR},
                 {"agg": "max", "col": "latency", "filter": ERR}],
      "group_by": ["host"]}


def _partial(keys, presence, fcount, fmax):
    return pa.record_batch({
        "host": pa.array(keys, type=pa.string()),
        "__presence": pa.array(presence, type=pa.int64()),
        "agg0": pa.array(presence, type=pa.int64()),
        "agg0_count": pa.array(presence, type=pa.int64()),
        "agg1": pa.array(fcount, type=pa.int64()),
        "agg1_count": pa.array(fcount, type=pa.int64()),
        "agg2": pa.array(fmax, type=pa.int64()),
        "agg2_count": pa.array(fcount, type=pa.int64()),
    })


# host a: filtered count 0 in one partial and > 0 in the other; host b: 0 in
# both; host c: only in one partial, 0 there
PART0 = (["a", "b", "c"], [3, 4, 2], [0, 0, 0], [None, None, None])
PART1 = (["a", "b"], [2, 5], [2, 0], [70, None])
MERGED = [["a", 5, 2, 70], ["b", 9, 0, None], ["c", 2, 0, None]]


def test_merge_partials_keeps_groups_with_filtered_count_zero():
    from parseable_amd.provider import merge_partials

    assert merge_partials([_partial(*PART0), _partial(*PART1)], MQ) == MERGED
    # the single-partial shortcut reads the value columns
    assert merge_partials([_partial(*PART0)], MQ) == [
        ["a", 3, 0, None], ["b", 4, 0, None], ["c", 2, 0, None]]
    # no group-by: always one row
    q = {"select": MQ["select"][1:]}
    b = pa.record_batch({"__presence": pa.array([4], type=pa.int64()),
                         "agg0": pa.array([0], type=pa.int64()),
                         "agg0_count": pa.array([0], type=pa.int64()),
                         "agg1": pa.array([None], type=pa.int64()),
                         "agg1_count": pa.array([0], type=pa.int64())})
    assert merge_partials([b], q) == [[0, None]]
    assert merge_partials([b, b], q) == [[0, None]]


def _rank_main(rank, world, port, q):
    import torch.distributed as dist

    from parseable_amd.dist import DistMerger

    dist.init_process_group(
        "gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        batch = _partial(*(PART0 if rank == 0 else PART1))
        m = DistMerger(MQ, device="cpu")
        m.setup(batch)
        q.put((rank, m.step(batch)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_gloo_world2_merge():
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
    results = dict(q.get() for _ in range(2))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert results[0] == results[1] == MERGED
