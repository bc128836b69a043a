"""WHERE trees (`query["where"]`: nested and / or groups), host side: the
node ABI, validation and normalisation, tree-aware pruning through the
native and the Python planner (GPUQ_FAKE_DEVICE — plan building is pure host
work), single-column LUT folding, the count fast path, the staging reader,
and the plain-Python reference of tests/where_common.py itself."""

import ctypes as C
import os
import re

import pytest

from tests import strpred_common as sc
from tests import where_common as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE, MIN = wc.BASE, wc.MIN
COUNT = [{"agg": "count_star"}]
L = wc.leaf


def in_file(i):
    """p_timestamp inside file i's minute (inclusive between)."""
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

    td = tmp_path_factory.mktemp("where_cpu_c6")
    info = gen_stream(str(td), "s", "c6", **wc.GEN)
    info["data"] = wc.load(info["files"])
    return info


@pytest.fixture(scope="module")
def provider(c6):
    from parseable_amd import GpuSession, StandardTableProvider

    return StandardTableProvider(c6["stream_dir"], GpuSession())


# ---- ABI ---------------------------------------------------------------

def test_lib_matches_header():
    from parseable_amd import _lib

    src = open(os.path.join(ROOT, "include", "gpuq.h")).read()
    m = re.search(r"typedef enum \{([^}]*)\} gpuq_node_kind;", src)
    names = [x.strip().partition("=")[0].strip() for x in m.group(1).split(",")]
    assert names == ["GPUQ_NODE_LEAF", "GPUQ_NODE_AND", "GPUQ_NODE_OR"]
    assert _lib.NODE_KINDS == {"leaf": 0, "and": 1, "or": 2}
    m = re.search(r"typedef struct \{([^}]*)\} gpuq_where_node;", src)
    fields = [f.split()[-1] for f in m.group(1).split(";") if f.strip()]
    assert fields == [n for n, _ in _lib.GpuqWhereNode._fields_]
    assert all(t is C.c_int32 for _, t in _lib.GpuqWhereNode._fields_)
    assert C.sizeof(_lib.GpuqWhereNode) == 12
    lib = _lib.load()
    for base in ("gpuq_plan_build", "gpuq_plan_build_from_stream"):
        decl = re.search(r"gpuq_plan\* %s_where\((.*?)\);" % base, src, re.S)
        assert decl, base
        assert decl.group(1).rstrip().endswith(
            "const gpuq_where_node* nodes, int32_t n_nodes")
        old, new = getattr(lib, base), getattr(lib, base + "_where")
        assert new.argtypes[:-2] == old.argtypes
        assert new.argtypes[-1] is C.c_int32
    assert re.search(r"int32_t gpuq_test_mask_ops\(gpuq_ctx\*, int32_t op", src)
    assert len(lib.gpuq_test_mask_ops.argtypes) == 9
    assert int(re.search(r"#define GPUQ_MASK_TEST_MARGIN (\d+)", src).group(1)) \
        == _lib.MASK_TEST_MARGIN
    assert int(re.search(r"#define GPUQ_MASK_TEST_SENTINEL (\w+)", src).group(1),
               16) == _lib.MASK_TEST_SENTINEL
    ops = re.search(r"enum \{ GPUQ_MASK_OR_RESET = (\d), GPUQ_MASK_AND = (\d) \}",
                    src)
    assert _lib.MASK_OPS == {"or_reset": int(ops.group(1)),
                             "and": int(ops.group(2))}


# ---- validation ----------------------------------------------------------

def _raw_build(provider, c6, preds, nodes, native):
    """Build a count(*) plan from a raw node list [(kind, parent, pred)];
    -> None when the plan builds, else the library's error text."""
    from parseable_amd import _lib
    from parseable_amd.provider import _build_c_projection, _build_c_query

    lib = _lib.load()
    sess = provider.session
    keep = []
    q = {"select": COUNT, "preds": preds}
    cpreds, np_, cgroup, ng, caggs, na = _build_c_query(q, keep)
    cproj, nproj, limit = _build_c_projection(q, keep)
    cn = (_lib.GpuqWhereNode * max(len(nodes), 1))()
    for i, (k, par, pr) in enumerate(nodes):
        cn[i].kind, cn[i].parent, cn[i].pred = k, par, pr
    if native:
        fc = C.c_int64(-1)
        plan = lib.gpuq_plan_build_from_stream_where(
            sess._ctx, c6["stream_dir"].encode(), cproj, nproj, cpreds, np_,
            cgroup, ng, caggs, na, C.c_int64(limit), C.byref(fc), cn, len(nodes))
        if not plan and fc.value != -1:
            return None
    else:
        files = (_lib.GpuqFile * len(c6["files"]))()
        pb = [p.encode() for p in c6["files"]]
        for i, b in enumerate(pb):
            files[i].path, files[i].row_groups, files[i].n_row_groups = b, None, -1
        plan = lib.gpuq_plan_build_where(
            sess._ctx, files, len(pb), cproj, nproj, cpreds, np_, cgroup, ng,
            caggs, na, C.c_int64(limit), cn, len(nodes))
    if plan:
        lib.gpuq_plan_destroy(plan)
        return None
    return sess._err()


LEAF, AND, OR = 0, 1, 2
P2 = [L("level", "eq", "ERROR"), L("latency", "lt", 1000)]

BAD_TREES = [
    ("root parent", P2, [(OR, 0, -1), (LEAF, 0, 0), (LEAF, 0, 1)],
     "parent must be -1"),
    ("forward parent", P2, [(OR, -1, -1), (LEAF, 2, 0), (LEAF, 0, 1)],
     "malformed parent link"),
    ("self parent", P2, [(OR, -1, -1), (LEAF, 1, 0), (LEAF, 0, 1)],
     "malformed parent link"),
    ("negative parent", P2, [(OR, -1, -1), (LEAF, -1, 0), (LEAF, 0, 1)],
     "malformed parent link"),
    ("leaf parent", P2, [(OR, -1, -1), (LEAF, 0, 0), (LEAF, 1, 1)],
     "is a leaf"),
    ("bad kind", P2, [(3, -1, -1), (LEAF, 0, 0), (LEAF, 0, 1)],
     "unknown node kind"),
    ("childless or", P2, [(AND, -1, -1), (LEAF, 0, 0), (LEAF, 0, 1), (OR, 0, -1)],
     "at least one condition or group"),
    ("childless and", P2, [(OR, -1, -1), (LEAF, 0, 0), (LEAF, 0, 1), (AND, 0, -1)],
     "at least one condition or group"),
    ("unused pred", P2, [(OR, -1, -1), (LEAF, 0, 0)], "used by no leaf"),
    ("double pred", P2, [(OR, -1, -1), (LEAF, 0, 0), (LEAF, 0, 1), (LEAF, 0, 0)],
     "more than one leaf"),
    ("pred out of range", P2, [(OR, -1, -1), (LEAF, 0, 0), (LEAF, 0, 2)],
     "names no predicate"),
]


@pytest.mark.parametrize("native", [True, False])
@pytest.mark.parametrize("name,preds,nodes,msg", BAD_TREES,
                         ids=[b[0] for b in BAD_TREES])
def test_validation_errors(provider, c6, native, name, preds, nodes, msg):
    err = _raw_build(provider, c6, preds, nodes, native)
    assert err is not None and msg in err, err


@pytest.mark.parametrize("native", [True, False])
def test_leaf_and_depth_limits(provider, c6, native):
    preds = [L("latency", "ne", i) for i in range(33)]
    nodes = [(OR, -1, -1)] + [(LEAF, 0, i) for i in range(33)]
    assert "more than 32 leaves" in _raw_build(provider, c6, preds, nodes, native)
    assert _raw_build(provider, c6, preds[:32], nodes[:33], native) is None

    def chain(n_or):
        """OR(leaf, AND(leaf, OR(leaf, AND(...)))) with n_or OR levels."""
        nodes, preds, parent = [], [], -1
        for d in range(n_or):
            nodes.append((OR, parent, -1))
            o = len(nodes) - 1
            nodes.append((LEAF, o, len(preds)))
            preds.append(L("latency", "lt", 1000 + d))
            nodes.append((AND, o, -1))
            a = len(nodes) - 1
            nodes.append((LEAF, a, len(preds)))
            preds.append(L("opt_i64", "gt", d))
            parent = a
        nodes.append((LEAF, parent, len(preds)))
        preds.append(L("level", "eq", "ERROR"))
        return preds, nodes

    preds, nodes = chain(5)
    assert "OR nesting depth above 4" in _raw_build(provider, c6, preds, nodes,
                                                     native)
    preds, nodes = chain(4)
    assert _raw_build(provider, c6, preds, nodes, native) is None
    # same-kind nesting flattens: five nested ORs are one OR of depth 1
    nodes, preds, parent = [], [], -1
    for d in range(5):
        nodes.append((OR, parent, -1))
        parent = len(nodes) - 1
        nodes.append((LEAF, parent, len(preds)))
        preds.append(L("latency", "lt", 1000 + d))
    nodes.append((LEAF, parent, len(preds)))
    preds.append(L("opt_i64", "gt", 5))
    assert _raw_build(provider, c6, preds, nodes, native) is None


def test_python_surface_errors(provider):
    from parseable_amd.provider import GpuqError

    with pytest.raises(GpuqError, match="exactly one key"):
        provider.scan({"select": COUNT, "where": {"and": [P2[0]], "or": [P2[1]]}})
    with pytest.raises(GpuqError, match="at least one condition or group"):
        provider.scan({"select": COUNT, "where": {"and": []}})
    with pytest.raises(GpuqError, match="at least one condition or group"):
        provider.scan({"select": COUNT,
                       "where": {"or": [P2[0], {"and": []}]}})
    # also inside a pure conjunction, which never reaches the library as nodes
    for native in (True, False):
        for where in ({"and": [P2[0], {"and": []}]},
                      {"and": [P2[0], {"and": [P2[1], {"or": []}]}]}):
            with pytest.raises(GpuqError, match="at least one condition or group"):
                _scan(provider, {"select": COUNT, "where": where}, native)


# ---- planning --------------------------------------------------------------

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


def _debug_lines(err):
    """Plan-debug text without the wall-clock phase lines."""
    return [ln for ln in err.splitlines()
            if ln.startswith("[gpuq") and not ln.rstrip().endswith(" ms")]


@pytest.mark.parametrize("native", [True, False])
def test_and_only_tree_is_the_flat_plan(provider, capfd, native):
    preds = [L("message", "icontains", "error"), L("level", "starts_with", "E"),
             L("latency", "lt", 500_000), L("opt_i64", "is_not_null")]
    tr = [BASE + 5_000, BASE + 2 * MIN + 1_000]
    flat = {"select": COUNT, "preds": preds, "time_range": tr}
    tree = {"select": COUNT, "time_range": tr,
            "where": {"and": [preds[0], {"and": [preds[1], {"and": [preds[2]]}]},
                              preds[3]]}}
    mixed = {"select": COUNT, "time_range": tr, "preds": preds[:2],
             "where": {"and": [preds[2], preds[3]]}}
    a = _scan(provider, flat, native, capfd)
    assert a[0] == "scan" and _debug_lines(a[2])
    for q in (tree, mixed):
        b = _scan(provider, q, native, capfd)
        assert b[:2] == a[:2]
        assert _debug_lines(b[2]) == _debug_lines(a[2])
        assert "[gpuq plan] where" not in b[2]


@pytest.mark.parametrize("native", [True, False])
def test_single_child_or_collapses(provider, capfd, native):
    a = _scan(provider, {"select": COUNT, "preds": [P2[1]]}, native, capfd)
    b = _scan(provider, {"select": COUNT, "where": {"or": [{"and": [P2[1]]}]}},
              native, capfd)
    assert b[:2] == a[:2] and _debug_lines(b[2]) == _debug_lines(a[2])


ROWS = wc.GEN["rows_per_file"]

PRUNE = [
    ("two files", {"where": {"or": [in_file(0), in_file(2)]}}, 2 * ROWS),
    ("time or value", {"where": {"or": [in_file(0),
                                         L("level", "contains", "E")]}}, 3 * ROWS),
    ("or and time_range",
     {"where": {"or": [in_file(0), in_file(2)]},
      "time_range": [BASE + 2 * MIN, BASE + 3 * MIN]}, ROWS),
    ("required is_null or eq",
     {"where": {"or": [L("latency", "is_null"), L("level", "eq", "ERROR")]}},
     3 * ROWS),
    ("and of ors", {"where": {"and": [{"or": [in_file(0), in_file(1)]},
                                      {"or": [in_file(1), in_file(2)]}]}}, ROWS),
    ("nested", {"where": {"or": [{"and": [in_file(0), L("latency", "lt", -5)]},
                                 in_file(1)]}}, ROWS),
]


@pytest.mark.parametrize("name,extra,rows", PRUNE, ids=[p[0] for p in PRUNE])
def test_pruning_is_a_tree_evaluation(provider, capfd, name, extra, rows):
    q = dict({"select": COUNT, "group_by": ["level"]}, **extra)
    a = _scan(provider, q, native=True, capfd=capfd)
    b = _scan(provider, q, native=False, capfd=capfd)
    assert a[:2] == b[:2] == ("scan", rows), (a[:2], b[:2])
    # the plan holds the tree (a plan that ignored `where` scans as much in
    # the cases that drop nothing) and every one of its leaves
    n_leaves = len(wc.leaves(extra["where"])) + ("time_range" in extra)
    for _, _, err in (a, b):
        assert len(re.findall(r"\[gpuq plan\] where \S.* contexts=\d+ depth=\d+",
                              err)) == 1, err[-1500:]
        assert len(re.findall(r"\[gpuq plan\] where pred \d+ ", err)) == n_leaves


IMPOSSIBLE = [
    {"or": [L("p_timestamp", "lt", BASE - 5), L("p_timestamp", "gt", BASE + 10 * MIN)]},
    {"or": [L("p_timestamp", "lt", BASE - 5), L("latency", "is_null")]},
    {"or": [L("latency", "is_null"),
            {"and": [L("level", "eq", "ERROR"), L("p_timestamp", "is_null")]}]},
]


@pytest.mark.parametrize("native", [True, False])
@pytest.mark.parametrize("where", IMPOSSIBLE)
def test_impossible_or_is_the_empty_relation(provider, native, where):
    for sel in (COUNT, [{"agg": "max", "col": "latency"}]):
        a = _scan(provider, {"select": sel, "where": where}, native)
        assert a[0] == "empty", a[:2]


@pytest.mark.parametrize("native", [True, False])
def test_count_fast_path_needs_a_flat_time_filter(provider, native):
    tr = [BASE, BASE + MIN]
    assert _scan(provider, {"select": COUNT, "time_range": tr}, native)[:2] == (
        "count", ROWS)
    for where in ({"or": [in_file(0), L("level", "eq", "ERROR")]},
                  {"or": [in_file(0), in_file(2)]},
                  {"and": [in_file(0), {"or": [L("latency", "lt", 5),
                                               L("message", "is_null")]}]}):
        a = _scan(provider, {"select": COUNT, "where": where}, native)
        assert a[0] == "scan", (where, a[:2])
        a = _scan(provider, {"select": COUNT, "where": where, "time_range": tr},
                  native)
        assert a[0] == "scan", (where, a[:2])


def _or_paths(err):
    return re.findall(r"\[gpuq plan\] or node=\d+ terms=(\d+) path=(\w+)", err)


@pytest.mark.parametrize("native", [True, False])
def test_folding(provider, capfd, native):
    q = {"select": COUNT, "where": {"or": [L("level", "eq", "ERROR"),
                                           L("level", "eq", "WARN"),
                                           L("level", "icontains", "bug")]}}
    _, _, err = _scan(provider, q, native, capfd)
    assert _or_paths(err) == [("3", "lut")], err[-1500:]
    assert re.search(r"\[gpuq plan\] where \(0 OR 1 OR 2\) contexts=1 depth=1", err)
    # message has PLAIN pages: the general path, one context per term
    q = {"select": COUNT, "where": {"or": [L("message", "contains", "error"),
                                           L("message", "contains", "timeout")]}}
    _, _, err = _scan(provider, q, native, capfd)
    assert _or_paths(err) == [("2", "mask")], err[-1500:]
    assert re.search(r"\[gpuq plan\] where \(0 OR 1\) contexts=3 depth=1", err)
    # a hash-mode column (tag as a group key)
    q = {"select": COUNT, "group_by": ["tag"],
         "where": {"or": [L("tag", "contains", "ag-0001"),
                          L("tag", "ends_with", "7")]}}
    _, _, err = _scan(provider, q, native, capfd)
    assert _or_paths(err) == [("2", "mask")], err[-1500:]
    assert "col=tag op=contains path=hash" in err
    # a null leaf keeps the group off the LUT; a nested single-column group
    # folds inside a general one
    q = {"select": COUNT, "where": {"or": [
        L("level", "is_null"),
        {"and": [L("latency", "lt", 1000),
                 {"or": [L("level", "eq", "ERROR"), L("level", "eq", "WARN")]}]}]}}
    _, _, err = _scan(provider, q, native, capfd)
    assert sorted(_or_paths(err)) == [("2", "lut"), ("2", "mask")], err[-1500:]
    assert re.search(r"where \(0 OR \(1 AND \(2 OR 3\)\)\) contexts=3 depth=2", err)


@pytest.mark.parametrize("native", [True, False])
def test_same_kind_nesting_leaves_one_or_line(provider, capfd, native):
    """Flattened groups leave nothing behind: one `or node` line per OR of the
    normalised tree, with the path the group really took."""
    A, B, C3 = (L("level", "eq", "ERROR"), L("level", "eq", "WARN"),
                L("level", "eq", "info"))
    q = {"select": COUNT, "where": {"or": [A, {"or": [B, {"or": [C3]}]}]}}
    _, _, err = _scan(provider, q, native, capfd)
    assert _or_paths(err) == [("3", "lut")], err[-1500:]
    assert re.search(r"where \(0 OR 1 OR 2\) contexts=1 depth=1", err)
    q = {"select": COUNT, "where": {"or": [
        L("latency", "lt", 1000),
        {"or": [L("opt_i64", "gt", 5), {"and": [{"and": [A, L("latency", "gt", 7)]},
                                               {"or": [{"or": [B, C3]}]}]}]}]}}
    _, _, err = _scan(provider, q, native, capfd)
    assert sorted(_or_paths(err)) == [("2", "lut"), ("3", "mask")], err[-1500:]
    assert re.search(
        r"where \(0 OR 1 OR \(2 AND 3 AND \(4 OR 5\)\)\) contexts=4 depth=2", err)


def test_pushdown_answer_for_groups():
    from parseable_amd.provider import supports_filters_pushdown

    got = supports_filters_pushdown([
        {"col": "p_timestamp", "op": "ge", "lit": BASE},
        {"or": [{"col": "p_timestamp", "op": "ge", "lit": BASE},
                {"col": "p_timestamp", "op": "lt", "lit": BASE + MIN}]},
        {"and": [{"col": "p_timestamp", "op": "ge", "lit": BASE}]}])
    assert got == ["exact", "inexact", "inexact"]


# ---- the reference against strpred_common ----------------------------------

CONJ = [
    [L("message", "icontains", "error"), L("level", "not_starts_with", "E")],
    [L("message", "is_null"), L("opt_i64", "is_not_null"),
     wc.ts_between(40_000, 140_000)],
    [L("tag", "ends_with", "7"), L("message", "not_contains", "e")],
]


@pytest.mark.parametrize("preds", CONJ)
def test_reference_conjunctions_agree_with_strpred(c6, preds):
    data = c6["data"]
    tr = [BASE + 10_000, BASE + 2 * MIN + 30_000]
    want = sc.selected(data, {"preds": preds, "time_range": tr})
    assert wc.selected(data, {"preds": preds, "time_range": tr}) == want
    assert wc.selected(data, {"where": {"and": preds}, "time_range": tr}) == want
    assert wc.selected(data, {"where": {"and": [preds[0], {"and": preds[1:]}]},
                              "time_range": tr}) == want
    assert 0 < len(want) < len(data["p_timestamp"])
    q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"}],
         "group_by": ["level"], "preds": preds, "time_range": tr}
    assert wc.expected(data, q) == sc.expected(data, q)


@pytest.mark.parametrize("a,b", [
    (L("message", "contains", "TIMEOUT"), L("level", "icontains", "warn")),
    (L("opt_i64", "is_null"), L("message", "ends_with", "r")),
    (wc.ts_between(40_000, 140_000), L("tag", "is_not_null")),
])
def test_reference_or_is_inclusion_exclusion(c6, a, b):
    data = c6["data"]
    na = len(sc.selected(data, {"preds": [a]}))
    nb = len(sc.selected(data, {"preds": [b]}))
    nab = len(sc.selected(data, {"preds": [a, b]}))
    assert len(wc.selected(data, {"where": {"or": [a, b]}})) == na + nb - nab
    assert 0 < nab < min(na, nb)


def test_random_trees_cover_every_path(c6):
    trees = wc.random_trees(c6["data"])
    assert len(trees) >= 40
    n_all = len(c6["data"]["p_timestamp"])
    for path in wc.PATHS:
        n = sum(any(wc.leaf_path(x) == path for x in wc.leaves(t))
                for t, _ in trees)
        assert n >= 5, (path, n)
    for t, n_sel in trees:
        assert 0 < n_sel < n_all
        assert len(wc.leaves(t)) <= 6
    assert trees == wc.random_trees(c6["data"])   # the seed fixes the list


# ---- staging leg -------------------------------------------------------------

@pytest.fixture(scope="module")
def staged(tmp_path_factory):
    """A staging-only stream (.arrows files alone): every row is read by
    StagingScanner on the host."""
    import json

    import pyarrow as pa

    from datagen.gen import gen_staging

    td = tmp_path_factory.mktemp("where_staging")
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


STAGE_TREES = [
    {"or": [L("level", "eq", "ERROR"), L("level", "eq", "warn")]},
    {"or": [L("message", "contains", "TIMEOUT"), L("opt_i64", "gt", 0)]},
    {"or": [L("f_f64", "lt", 0.2), {"and": [L("f_f64", "is_null"),
                                             L("level", "eq", "ERROR")]}]},
    {"and": [{"or": [L("message", "is_null"), L("latency", "lt", 300_000)]},
             {"or": [L("tag", "starts_with", "Tag"), L("level", "is_null")]}]},
    {"or": [L("opt_i64", "is_null"),
            {"and": [L("message", "not_contains", "e"),
                     {"or": [L("latency", "ge", 900_000),
                             L("level", "icontains", "info")]}]}]},
]


@pytest.mark.parametrize("tree", STAGE_TREES)
def test_staging_leg(staged, tree):
    from oracle.compare import assert_rows_equal
    from parseable_amd import Query, StandardTableProvider

    sdir, stg, st, data = staged
    prov = StandardTableProvider(sdir, None, staging_dir=stg, now_ms=st["max_ts"])
    q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"}],
         "group_by": ["level"], "where": tree,
         "preds": [L("latency", "ne", 7)]}
    rows, _ = Query(prov).execute(dict(q))
    assert_rows_equal(rows, wc.expected(data, q), f"staging {tree}")
    assert 0 < len(wc.selected(data, q)) < len(data["p_timestamp"])
    q = {"select_cols": ["p_timestamp", "level", "latency"], "where": tree,
         "limit": 50}
    rows, _ = Query(prov).execute(dict(q))
    want = wc.expected(data, q)
    assert [r[0] for r in rows] == [r[0] for r in want]
