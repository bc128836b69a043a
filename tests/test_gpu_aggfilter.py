"""Per-aggregate FILTER (`{"agg": ..., "filter": ...}` in query["select"]) on
the GPU: every leaf evaluation path as a filter, every aggregate kind under a
filter, group presence, several filters in one plan, filter trees, chunk-stats
elision inside a filter, the kernel each shape runs, and seeded random
queries. Expected values come from tests/aggfilter_common.py (plain Python
over the parquet files); paths and kernels are read from the GPUQ_PLAN_DEBUG
lines
  [gpuq plan] agg <i> filter <expr> ctx=<k> depth=<d>
  [gpuq plan] where pred <p> col=<c> op=<o> ctx=<k> rowgroups: eval=.. elided=..
  [gpuq exec] part <p>: agg=fcount|general+filter filters=<n> filter_bufs=<n>
      n_groups=<G> table_bytes=<B>

Data: c6 (60,000 rows, three files), a 1003-row c6 stream in 400-row files
(row counts that are no multiple of 4: the tail loops run), c6 streams of 1,
3, 4, 5 and 1027 rows, and a 5,000-row c1 stream (1000 hosts). All comparisons
are exact, f64 sums within 1 ULP (oracle.compare)."""

import os
import random
import re

import pytest

from tests import aggfilter_common as ac
from tests import strpred_common as sc
from tests import where_common as wc

pytestmark = pytest.mark.gpu

BASE, MIN = wc.BASE, wc.MIN
L = wc.leaf
STAR = {"agg": "count_star"}

ERR = L("level", "eq", "ERROR")
NOPE = L("level", "eq", "NOPE")
SLOW = L("latency", "ge", 900_000)
FAST = L("latency", "lt", 300_000)
TMO = L("message", "icontains", "timeout")
HALF = L("f_f64", "lt", 0.5)
KNOBS = ("GPUQ_NO_FCOUNT", "GPUQ_DISTINCT_FORCE_HASH", "GPUQ_DISTINCT_LDS_BITS")


def F(agg, f, col=None):
    a = {"agg": agg, "filter": f}
    if col:
        a["col"] = col
    return a


def _stream(tmp_path_factory, name, config, **gen):
    from datagen.gen import gen_stream

    td = tmp_path_factory.mktemp(name)
    info = gen_stream(str(td), "s", config, **gen)
    info["data"] = sc.load(info["files"])
    return info


@pytest.fixture(scope="module")
def c6(tmp_path_factory):
    return _stream(tmp_path_factory, "aggfilter_c6", "c6", **wc.GEN)


@pytest.fixture(scope="module")
def c6_odd(tmp_path_factory):
    return _stream(tmp_path_factory, "aggfilter_c6_odd", "c6", **wc.GEN_ODD)


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    return {n: _stream(tmp_path_factory, "aggfilter_c6_%d" % n, "c6", rows=n,
                       rows_per_file=400, data_page_size=65536)
            for n in (1, 3, 4, 5, 1027)}


@pytest.fixture(scope="module")
def c1(tmp_path_factory):
    return _stream(tmp_path_factory, "aggfilter_c1", "c1", rows=5_000)


@pytest.fixture(scope="module")
def session():
    from parseable_amd import GpuSession

    return GpuSession()


def _gpu(info, session, q, capfd, **env):
    from parseable_amd import Query, StandardTableProvider

    for k in KNOBS:
        assert k not in os.environ
    os.environ["GPUQ_PLAN_DEBUG"] = "1"
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        capfd.readouterr()
        prov = StandardTableProvider(info["stream_dir"], session)
        rows, _ = Query(prov).execute(dict(q))
        err = capfd.readouterr().err
    finally:
        os.environ.pop("GPUQ_PLAN_DEBUG", None)
        for k in env:
            os.environ.pop(k, None)
    return rows, err


def _check(info, session, q, capfd, **env):
    from oracle.compare import assert_rows_equal

    rows, err = _gpu(info, session, q, capfd, **env)
    assert_rows_equal(rows, ac.expected(info["data"], q), f"GPU vs python: {q}")
    return rows, err


def _agg_path(err):
    m = re.findall(r"\[gpuq exec\] part 0: agg=(\S+) filters=(\d+) "
                   r"filter_bufs=(\d+) n_groups=(\d+) table_bytes=(\d+)", err)
    assert len(m) == 1, err[-1500:]
    return m[0][0], int(m[0][1]), int(m[0][2]), int(m[0][4])


def _n(data, node):
    return len(ac.node_rows(data, node))


# ---- every leaf path as a count(*) filter ------------------------------------------

SHAPES = {"nokey": [], "level": ["level"], "tag": ["tag"]}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("path", wc.PATHS)
def test_leaf_paths(c6, session, capfd, path, shape):
    data = c6["data"]
    n_all = len(data["p_timestamp"])
    leaf = next(x for x in wc.POOL[path] if 0 < _n(data, x) < n_all)
    q = {"select": [STAR, F("count_star", leaf)], "group_by": SHAPES[shape]}
    rows, err = _check(c6, session, q, capfd)
    # no WHERE: the first column is the whole group, the second is less
    nk = len(SHAPES[shape])
    assert sum(r[nk] for r in rows) == n_all
    assert sum(r[nk + 1] for r in rows) == _n(data, leaf)
    assert re.search(r"\[gpuq plan\] agg 1 filter 0 ctx=1 depth=0", err), err[-1500:]
    assert re.search(r"\[gpuq plan\] where pred 0 col=%s op=%s ctx=1 " % (
        leaf["col"], leaf["op"]), err), err[-1500:]
    kernel, nf, _, _ = _agg_path(err)
    assert (kernel, nf) == ("fcount" if nk == 1 else "general+filter", 1)
    # the path the leaf took
    if leaf["op"] in sc.STR_OPS and (leaf["col"] != "tag" or shape == "tag"):
        want = {"level": "lut", "message": "lut+window", "tag": "hash"}[leaf["col"]]
        assert re.search(r"\[gpuq plan\] pred 0 col=%s op=%s path=%s\n" % (
            leaf["col"], leaf["op"], re.escape(want)), err), err[-1500:]
    if path == "nulltask":
        assert re.search(r"\[gpuq plan\] pred 0 col=%s op=%s path=nulltask " % (
            leaf["col"], leaf["op"]), err), err[-1500:]
    # per row group (one per file): evaluated per row, or proven by chunk stats
    m = re.search(r"\[gpuq plan\] where pred 0 col=\S+ op=\S+ ctx=1 rowgroups: "
                  r"eval=(\d+) elided=(\d+)", err)
    ev = (int(m.group(1)), int(m.group(2)))
    if path == "between":
        assert ev == (2, 1), ev     # file 1 lies inside the range
    elif path != "nulltask":
        assert ev == (3, 0), ev
    else:
        assert sum(ev) == 3, ev
    # a compare leaf (k_cmp_i64 over the decoded column) has no string / null
    # path line and no mask task; a dict-LUT leaf decodes `level` into its mask
    # whatever the key is
    if path in ("i64", "f64", "between"):
        assert not re.search(r"\[gpuq plan\] pred 0 ", err), err[-1500:]
        assert leaf["col"] not in ("level", "message", "tag")
    if path == "lut" and shape != "level":
        assert re.search(r"\[gpuq exec\] part 0: dict decode col=level ", err)


# ---- every aggregate kind under a filter --------------------------------------------

KINDS = [
    ("count", [F("count", SLOW, "opt_i64"), {"agg": "count", "col": "opt_i64"}]),
    ("sum i64", [F("sum", ERR, "opt_i64"), F("sum", SLOW, "latency")]),
    ("sum f64", [F("sum", SLOW, "f_f64"), {"agg": "sum", "col": "f_f64"},
                 F("sum", TMO, "f_f64")]),
    ("min max i64", [F("min", ERR, "latency"), F("max", HALF, "opt_i64")]),
    ("min max f64", [F("min", SLOW, "f_f64"), F("max", ERR, "f_f64")]),
    ("min max rank", [F("min", L("level", "ge", "Info"), "level"),
                      F("max", L("latency", "lt", 20_000), "level")]),
    ("min max strref", [F("min", SLOW, "tag"), F("max", ERR, "tag")]),
    ("avg", [F("avg", SLOW, "latency"), F("avg", ERR, "f_f64"),
             {"agg": "avg", "col": "latency"}]),
]


@pytest.mark.parametrize("gb", [[], ["level"]], ids=["nokey", "level"])
@pytest.mark.parametrize("name,select", KINDS, ids=[k[0] for k in KINDS])
def test_aggregate_kinds(c6_odd, session, capfd, name, select, gb):
    q = {"select": [STAR] + select, "group_by": gb, "preds": [L("latency", "ne", 7)]}
    _, err = _check(c6_odd, session, q, capfd)
    assert _agg_path(err)[0] == "general+filter"
    # the filters matter
    from oracle.compare import rows_equal

    assert not rows_equal(ac.expected(c6_odd["data"], q),
                          ac.expected(c6_odd["data"], ac.strip(q)))


def test_aggregate_kinds_together(c6, session, capfd):
    q = {"select": [STAR] + [a for _, sel in KINDS for a in sel][:7],
         "group_by": ["level"], "where": {"or": [HALF, L("opt_i64", "is_null")]}}
    _check(c6, session, q, capfd)


DISTINCT = [("lds", {}, "bitmap", "lds"),
            ("global", {"GPUQ_DISTINCT_LDS_BITS": 0}, "bitmap", "global"),
            ("hash", {"GPUQ_DISTINCT_FORCE_HASH": 1}, "hash", None)]


@pytest.mark.parametrize("info_name", ["c6", "c6_odd"])
@pytest.mark.parametrize("name,env,path,mark", DISTINCT, ids=[d[0] for d in DISTINCT])
def test_count_distinct(request, session, capfd, name, env, path, mark, info_name):
    info = request.getfixturevalue(info_name)
    q = {"select": [F("count_distinct", SLOW, "sparse"),
                    {"agg": "count_distinct", "col": "sparse"},
                    F("count_distinct", NOPE, "sparse")],
         "group_by": ["level"], "preds": [FAST if info_name == "c6" else HALF]}
    rows, err = _check(info, session, q, capfd, **env)
    got = re.findall(r"distinct agg=(\d) col=sparse path=(\w+) groups=\d+ "
                     r"card=\d+ pairs=\d+(?: mark=(\S+))?", err)
    assert got == [(str(i), path, mark or "") for i in range(3)], err[-1500:]
    assert any(r[1] < r[2] for r in rows) and all(r[3] == 0 for r in rows)


# ---- groups come from WHERE alone ----------------------------------------------------

def test_group_whose_rows_all_fail_the_filter_stays(c6_odd, session, capfd):
    data = c6_odd["data"]
    sel = [STAR, F("count_star", NOPE), F("count", NOPE, "opt_i64"),
           F("sum", NOPE, "latency"), F("sum", NOPE, "f_f64"),
           F("min", NOPE, "level"), F("avg", NOPE, "latency"),
           F("count_distinct", NOPE, "tag")]
    plain = wc.expected(data, {"select": [STAR], "group_by": ["level"],
                               "preds": [SLOW]})
    assert len(plain) > 3
    rows, _ = _check(c6_odd, session, {"select": sel, "group_by": ["level"],
                                       "preds": [SLOW]}, capfd)
    assert rows == [r + [0, 0, None, None, None, None, 0] for r in plain]
    # with no group-by there is always one row
    rows, _ = _check(c6_odd, session, {"select": sel, "preds": [SLOW]}, capfd)
    assert rows == [[_n(data, SLOW), 0, 0, None, None, None, None, 0]]
    rows, _ = _check(c6_odd, session, {"select": sel[1:], "preds": [NOPE]}, capfd)
    assert rows == [[0, 0, None, None, None, None, 0]]


def test_filter_equal_to_where_and_disjoint_from_it(c6_odd, session, capfd):
    data = c6_odd["data"]
    where = {"or": [ERR, {"and": [SLOW, HALF]}]}
    sel = [{"agg": "count_star"}, {"agg": "max", "col": "latency"},
           {"agg": "sum", "col": "f_f64"}]
    for gb in ([], ["level"]):
        plain = wc.expected(data, {"select": sel, "group_by": gb, "where": where})
        nk = len(gb)
        same = [F(a["agg"], where, a.get("col")) for a in sel]
        rows, _ = _check(c6_odd, session, {"select": same, "group_by": gb,
                                           "where": where}, capfd)
        from oracle.compare import assert_rows_equal

        assert_rows_equal(rows, plain, "a filter equal to WHERE changes nothing")
        # disjoint: WHERE level = ERROR, filter level <> ERROR
        q = {"select": [STAR] + [F(a["agg"], L("level", "ne", "ERROR"), a.get("col"))
                                 for a in sel],
             "group_by": gb, "preds": [ERR]}
        rows, _ = _check(c6_odd, session, q, capfd)
        assert [r[nk:] for r in rows] == [[_n(data, ERR), 0, None, None]]


# ---- several filters ---------------------------------------------------------------------

def test_max_aggs_each_with_its_own_filter(c6, session, capfd):
    fs = [ERR, SLOW, TMO, HALF, L("opt_i64", "is_null"), {"or": [ERR, FAST]},
          L("tag", "starts_with", "Tag"), wc.ts_between(40_000, 140_000)]
    kinds = [("count_star", None), ("max", "latency"), ("count_star", None),
             ("sum", "f_f64"), ("count", "f_f64"), ("min", "opt_i64"),
             ("count_star", None), ("avg", "latency")]
    q = {"select": [F(k, f, c) for (k, c), f in zip(kinds, fs)],
         "group_by": ["level"], "preds": [L("latency", "ne", 7)]}
    _, err = _check(c6, session, q, capfd)
    assert _agg_path(err)[:3] == ("general+filter", 8, 8)
    assert len(re.findall(r"\[gpuq plan\] agg \d filter ", err)) == 8
    # eight count(*): the count-only kernel with eight filter buffers
    q = {"select": [F("count_star", f) for f in fs], "group_by": ["level"]}
    _, err = _check(c6, session, q, capfd)
    assert _agg_path(err)[:3] == ("fcount", 8, 8)


def test_shared_filter_and_filtered_next_to_unfiltered(c6_odd, session, capfd):
    q = {"select": [F("count_star", SLOW), F("max", SLOW, "opt_i64"),
                    {"agg": "max", "col": "opt_i64"},
                    F("sum", ERR, "latency"), {"agg": "sum", "col": "latency"}],
         "group_by": ["level"], "preds": [HALF]}
    rows, _ = _check(c6_odd, session, q, capfd)
    assert any(r[2] != r[3] for r in rows)


# ---- filter trees ----------------------------------------------------------------------------

def _or_lines(err):
    return re.findall(r"\[gpuq plan\] or node=\d+ terms=(\d+) path=(\w+)", err)


def test_or_filter_folds_into_one_lut(c6, session, capfd):
    f = {"or": [ERR, L("level", "starts_with", "W"), L("level", "eq", "info")]}
    q = {"select": [STAR, F("count_star", f)], "group_by": ["tag"]}
    _, err = _check(c6, session, q, capfd)
    assert _or_lines(err) == [("3", "lut")], err[-1500:]
    assert re.search(r"where bufs=0 combines=0", err), err[-1500:]
    assert len(re.findall(r"where pred \d col=level op=\S+ ctx=-1 ", err)) == 3


def test_depth_two_or_filter(c6_odd, session, capfd):
    f = {"or": [ERR, {"and": [SLOW, {"or": [HALF, L("opt_i64", "is_null")]}]}]}
    q = {"select": [STAR, F("count_star", f), F("max", f, "latency")],
         "group_by": ["level"]}
    _, err = _check(c6_odd, session, q, capfd)
    # the tree is built once per aggregate that carries it
    assert _or_lines(err) == [("2", "mask")] * 4, err[-1500:]
    assert re.search(r"agg 1 filter \S.* ctx=\d+ depth=2", err), err[-1500:]
    assert re.search(r"where bufs=4 ", err), err[-1500:]


def test_where_or_and_two_or_filters_share_the_level_buffers(c6, session, capfd):
    q = {"select": [STAR, F("count_star", {"or": [ERR, SLOW]}),
                    F("sum", {"or": [TMO, HALF]}, "latency")],
         "group_by": ["level"],
         "where": {"or": [FAST, L("message", "is_null")]}}
    _, err = _check(c6, session, q, capfd)
    assert _or_lines(err) == [("2", "mask")] * 3, err[-1500:]
    # one acc / tmp pair serves the WHERE evaluation and both filters
    assert re.search(r"where bufs=2 combines=6\n", err), err[-1500:]


# ---- chunk-stats elision inside a filter ------------------------------------------------------

@pytest.mark.parametrize("bi", [0, 1])
def test_elision_inside_a_filter(c6, session, capfd, bi):
    f = wc.POOL["between"][bi]
    q = {"select": [STAR, F("count_star", f), F("min", f, "p_timestamp")],
         "group_by": ["level"]}
    _, err = _check(c6, session, q, capfd)
    m = re.search(r"where pred 0 col=p_timestamp op=between ctx=1 rowgroups: "
                  r"eval=(\d+) elided=(\d+)", err)
    # a row group (one per file) is proven when all its timestamps lie inside
    data = c6["data"]
    proven = 0
    for fi in range(3):
        ts = [t for t, x in zip(data["p_timestamp"], data["__file"]) if x == fi]
        proven += f["lo"] <= min(ts) and max(ts) <= f["hi"]
    assert m and (int(m.group(1)), int(m.group(2))) == (3 - proven, proven), (
        proven, err[-1500:])
    assert proven > 0 or bi == 1
    # a filter proven for every row group passes no buffer at all
    q = {"select": [STAR, F("count_star", L("p_timestamp", "ge", BASE))],
         "group_by": ["level"]}
    rows, err = _check(c6, session, q, capfd)
    assert all(r[1] == r[2] for r in rows)
    assert "agg=general filters=1 filter_bufs=0" in err, err[-1500:]


# ---- which kernel ran ----------------------------------------------------------------------------

def test_error_rate_shape_runs_fcount(c6_odd, session, capfd):
    q = {"select": [STAR, F("count_star", ERR), F("count_star", SLOW)],
         "group_by": ["tag"], "preds": [HALF]}
    rows, err = _check(c6_odd, session, q, capfd)
    assert _agg_path(err)[0] == "fcount"
    rows2, err2 = _check(c6_odd, session, q, capfd, GPUQ_NO_FCOUNT=1)
    assert _agg_path(err2)[0] == "general+filter"
    assert rows2 == rows


def test_fcount_without_lds(c1, session, capfd):
    fs = [L("level", "eq", "ERROR"), L("latency", "ge", 500_000),
          L("level", "ne", "INFO"), L("latency", "lt", 100_000),
          {"or": [L("level", "eq", "WARN"), L("latency", "ge", 900_000)]}]
    q = {"select": [STAR, STAR, STAR] + [F("count_star", f) for f in fs],
         "group_by": ["host"]}
    rows, err = _check(c1, session, q, capfd)
    kernel, nf, _, table_bytes = _agg_path(err)
    assert (kernel, nf) == ("fcount", 5) and table_bytes > 64 * 1024
    assert len(rows) > 500
    rows2, err2 = _check(c1, session, q, capfd, GPUQ_NO_FCOUNT=1)
    assert _agg_path(err2)[0] == "general+filter" and rows2 == rows


def test_two_keys_run_the_general_kernel(c6_odd, session, capfd):
    q = {"select": [STAR, F("count_star", SLOW)], "group_by": ["level", "sparse"]}
    _, err = _check(c6_odd, session, q, capfd)
    assert _agg_path(err)[0] == "general+filter"


# ---- unfiltered plans ------------------------------------------------------------------------------

def test_headline_shape_keeps_its_fused_path(c1, session, capfd):
    head = {"select": [STAR, {"agg": "max", "col": "latency"}],
            "group_by": ["host"]}
    rows, err = _check(c1, session, head, capfd)
    assert "fused_count=0 fused_valagg=1" in err
    assert not re.search(r"\[gpuq plan\] agg \d filter|agg=\S+ filters=", err)
    q = dict(head, select=head["select"] + [F("count_star", L("level", "eq", "ERROR"))])
    rows2, err2 = _check(c1, session, q, capfd)
    assert "fused_count=0 fused_valagg=0" in err2
    assert [r[:3] for r in rows2] == rows
    count = {"select": [STAR], "group_by": ["host"]}
    _, err = _check(c1, session, count, capfd)
    assert "fused_count=1" in err


# ---- tiny streams ------------------------------------------------------------------------------------

@pytest.mark.parametrize("gb", [[], ["level"]], ids=["nokey", "level"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1027])
def test_tiny_streams(tiny, session, capfd, n, gb):
    q = {"select": [STAR, F("count_star", HALF), F("max", FAST, "latency"),
                    F("sum", HALF, "f_f64")], "group_by": gb}
    rows, _ = _check(tiny[n], session, q, capfd)
    assert sum(r[len(gb)] for r in rows) == n
    q = {"select": [STAR, F("count_star", HALF)], "group_by": ["level"]}
    _, err = _check(tiny[n], session, q, capfd)
    assert _agg_path(err)[0] == "fcount"


# ---- random queries -------------------------------------------------------------------------------------

N_RANDOM = 48
AGG_POOL = [("count_star", None), ("count", "opt_i64"), ("sum", "latency"),
            ("sum", "f_f64"), ("min", "opt_i64"), ("max", "f_f64"),
            ("min", "level"), ("max", "tag"), ("avg", "latency"),
            ("count_distinct", "level"), ("count_distinct", "opt_i64")]


_TREES = {}


def _random_query(data, i):
    """Seeded: a where_common.random_trees tree as WHERE, one to three more as
    filters on random aggregate kinds. The tree pools are built once per data
    set."""
    if id(data) not in _TREES:
        _TREES[id(data)] = (
            [t for t, _ in wc.random_trees(data, seed=5150, want=N_RANDOM)],
            [t for t, _ in wc.random_trees(data, seed=9091, want=3 * N_RANDOM,
                                           max_leaves=4)])
    wtrees, ftrees_all = _TREES[id(data)]
    rng = random.Random(977 + i)
    where = wtrees[i]
    ftrees = ftrees_all[3 * i:3 * i + 3]
    select = [STAR]
    for f in ftrees[:rng.randint(1, 3)]:
        kind, col = rng.choice(AGG_POOL)
        select.append(F(kind, f, col))
        if rng.random() < 0.3:   # the same aggregate unfiltered next to it
            select.append({k: v for k, v in select[-1].items() if k != "filter"})
    gb = rng.choice([[], ["level"], ["tag"], ["level", "sparse"]])
    return {"select": select, "group_by": gb, "where": where}


@pytest.mark.parametrize("i", range(N_RANDOM))
def test_random_queries(c6, c6_odd, session, capfd, i):
    info = c6 if i % 2 else c6_odd
    q = _random_query(info["data"], i)
    n_leaves = len(wc.leaves(q["where"])) + sum(
        len(wc.leaves(a["filter"])) for a in q["select"] if "filter" in a)
    assert n_leaves <= 32
    _, err = _check(info, session, q, capfd)
    assert _agg_path(err)[1] == sum("filter" in a for a in q["select"])
