"""WHERE trees (`query["where"]`: nested and / or groups) on the GPU: the two
mask-combine kernels through gpuq_test_mask_ops, OR groups over every leaf
evaluation path, tree shapes, every consumer of the selection mask, and
seeded random trees. Expected values come from tests/where_common.py (plain
Python over the parquet files); the path a group took is read from the
GPUQ_PLAN_DEBUG lines
  [gpuq plan] where <expr> contexts=<n> depth=<d>
  [gpuq plan] or node=<i> terms=<k> path=lut|mask
  [gpuq exec] part <p>: where bufs=<n> combines=<launches>

Data: c6 (60,000 rows, three files; `level` dict-only, `message` dict +
PLAIN pages, `tag` PLAIN pages, half of `opt_i64` and a fifth of `f_f64`
NULL); a 1003-row c6 stream in 400-row files (row ranges that are no multiple
of 16)."""

import itertools
import os
import random
import re

import pytest

from tests import strpred_common as sc
from tests import where_common as wc

pytestmark = pytest.mark.gpu

BASE, MIN = wc.BASE, wc.MIN
COUNT = [{"agg": "count_star"}]
L = wc.leaf


@pytest.fixture(scope="module")
def c6(tmp_path_factory):
    from datagen.gen import gen_stream

    td = tmp_path_factory.mktemp("where_c6")
    info = gen_stream(str(td), "s", "c6", **wc.GEN)
    info["data"] = wc.load(info["files"])
    return info


@pytest.fixture(scope="module")
def c6_odd(tmp_path_factory):
    from datagen.gen import gen_stream

    td = tmp_path_factory.mktemp("where_c6_odd")
    info = gen_stream(str(td), "s", "c6", **wc.GEN_ODD)
    info["data"] = wc.load(info["files"])
    return info


@pytest.fixture(scope="module")
def session():
    from parseable_amd import GpuSession

    return GpuSession()


# ---- the two kernels --------------------------------------------------------

@pytest.mark.parametrize("op", ["or_reset", "and"])
@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 255, 4095, 4096, 4097, 65539])
def test_mask_ops(session, op, n):
    from parseable_amd import _lib

    M, S = _lib.MASK_TEST_MARGIN, _lib.MASK_TEST_SENTINEL
    rng = random.Random(1000 * n + len(op))
    a = bytes(rng.getrandbits(1) for _ in range(n))
    b = bytes(rng.getrandbits(1) for _ in range(n))
    if op == "or_reset":
        want_a = bytes(x | y for x, y in zip(a, b))
        want_b = b"\x01" * n
    else:
        want_a = bytes(x & y for x, y in zip(a, b))
        want_b = b
    for a_lead, b_lead in itertools.product([0, 1, 15], repeat=2):
        out_a, out_b = _lib.mask_ops(session._ctx, op, a, b, a_lead, b_lead)
        for out, lead, want in ((out_a, a_lead, want_a), (out_b, b_lead, want_b)):
            assert len(out) == 2 * M + lead + n
            assert out[M + lead:M + lead + n] == want, (a_lead, b_lead)
            # every sentinel byte before and after the data is untouched
            assert out[:M + lead] == bytes([S]) * (M + lead), (a_lead, b_lead)
            assert out[M + lead + n:] == bytes([S]) * M, (a_lead, b_lead)


# ---- running a query ----------------------------------------------------------

def _gpu(info, session, q, capfd, py_planner=False):
    from parseable_amd import Query, StandardTableProvider

    os.environ["GPUQ_PLAN_DEBUG"] = "1"
    if py_planner:
        os.environ["GPUQ_PY_PLANNER"] = "1"
    try:
        capfd.readouterr()
        prov = StandardTableProvider(info["stream_dir"], session)
        rows, _ = Query(prov).execute(dict(q))
        err = capfd.readouterr().err
    finally:
        os.environ.pop("GPUQ_PLAN_DEBUG", None)
        os.environ.pop("GPUQ_PY_PLANNER", None)
    return rows, err


def _or_paths(err):
    return [p for _, p in re.findall(
        r"\[gpuq plan\] or node=\d+ terms=(\d+) path=(\w+)", err)]


def _check(info, session, q, capfd, **kw):
    """Run q, compare with the reference exactly, require a non-vacuous
    selection (some, not all, of the rows in the time range)."""
    from oracle.compare import assert_rows_equal

    data = info["data"]
    n_sel = len(wc.selected(data, q))
    n_range = len(wc.selected(data, {"time_range": q.get("time_range")}))
    assert 0 < n_sel < n_range, (q, n_sel, n_range)
    rows, err = _gpu(info, session, q, capfd, **kw)
    assert_rows_equal(rows, wc.expected(data, q), f"GPU vs python: {q}")
    return rows, err


# ---- an OR of two leaves for every pair of evaluation paths ------------------

_SEL = {}


def _n(data, node):
    key = (id(data), repr(node))
    if key not in _SEL:
        _SEL[key] = len(wc.selected(data, {"where": node}))
    return _SEL[key]


def _pick_pair(data, pool_a, pool_b):
    """Literals chosen on the CPU: the OR selects more than either term, not
    what their AND selects, and not everything."""
    n_all = len(data["p_timestamp"])
    for a, b in itertools.product(pool_a, pool_b):
        if a == b:
            continue
        n_or = _n(data, {"or": [a, b]})
        if (0 < n_or < n_all and n_or > _n(data, a) and n_or > _n(data, b)
                and n_or != _n(data, {"and": [a, b]})):
            return a, b
    raise AssertionError("no literal pair meets the conditions")


PAIRS = list(itertools.combinations_with_replacement(wc.PATHS, 2))


@pytest.mark.parametrize("pa,pb", PAIRS, ids=["%s|%s" % p for p in PAIRS])
def test_or_of_two_paths(c6, session, capfd, pa, pb):
    data = c6["data"]
    a, b = _pick_pair(data, wc.POOL[pa], wc.POOL[pb])
    q = wc.query_for({"or": [a, b]})
    _, err = _check(c6, session, q, capfd)
    folded = pa == pb == "lut"          # both on `level`: one LUT
    assert _or_paths(err) == ["lut" if folded else "mask"], err[-1500:]
    m = re.search(r"\[gpuq exec\] part 0: where bufs=(\d+) combines=(\d+)", err)
    assert m and (m.group(1), m.group(2)) == (("0", "0") if folded
                                              else ("2", "2")), err[-1500:]
    # the leaves took the paths the pool names them for
    for x, path in ((a, pa), (b, pb)):
        if path in ("lut", "lut+window", "hash") and x["op"] in sc.STR_OPS:
            assert re.search(r"col=%s op=%s path=%s\n" % (
                x["col"], x["op"], re.escape(path)), err), (x, err[-1500:])
        if path == "nulltask":
            assert re.search(r"col=%s op=%s path=nulltask " % (
                x["col"], x["op"]), err), (x, err[-1500:])
    # elision holds under the OR: file 1 lies inside the first between range,
    # so its row group is proven for that leaf and only the two boundary row
    # groups evaluate it per row
    leaf_lines = re.findall(
        r"\[gpuq plan\] where pred (\d+) col=(\S+) op=(\S+) ctx=(-?\d+) "
        r"rowgroups: eval=(\d+) elided=(\d+)", err)
    assert [(int(i), c, o) for i, c, o, _, _, _ in leaf_lines] == [
        (0, a["col"], a["op"]), (1, b["col"], b["op"])], err[-1500:]
    for x, ln in zip((a, b), leaf_lines):
        assert int(ln[3]) == (-1 if folded else 1 + (x is b)), ln
        if x == wc.POOL["between"][0]:
            assert (ln[4], ln[5]) == ("2", "1"), ln
    if "between" in (pa, pb):
        assert wc.POOL["between"][0] in (a, b)
        if "hash" not in (pa, pb):
            q2 = dict(q, select=COUNT + [{"agg": "min", "col": "p_timestamp"}])
            _check(c6, session, q2, capfd)


# ---- shapes ---------------------------------------------------------------------

A = L("level", "eq", "ERROR")
B = L("message", "icontains", "timeout")
Cc = L("latency", "lt", 300_000)
D = L("opt_i64", "gt", 0)
E = L("message", "is_null")
F = L("level", "not_starts_with", "E")

SHAPES = {
    "(A or B) and (C or D)": {"and": [{"or": [A, B]}, {"or": [Cc, D]}]},
    "A or (B and C)": {"or": [A, {"and": [B, Cc]}]},
    "depth 3": {"or": [A, {"and": [Cc, {"or": [B, {"and": [D, {"or": [E, F]}]}]}]}]},
    "same column and op in two contexts": {"or": [
        {"and": [L("message", "contains", "TIMEOUT"), L("latency", "lt", 500_000)]},
        {"and": [L("message", "contains", "rror"), L("latency", "ge", 500_000)]}]},
    "same lut column in two contexts": {"or": [
        {"and": [L("level", "eq", "ERROR"), L("latency", "lt", 500_000)]},
        {"and": [L("level", "eq", "warn"), L("latency", "ge", 500_000)]}]},
    "five terms": {"or": [L("level", "eq", "ERROR"),
                          L("message", "ends_with", "TIMEOUT"),
                          L("latency", "lt", 50_000),
                          L("opt_i64", "gt", 800_000_000),
                          L("level", "is_null")]},
    "null-bearing column under or": {"or": [L("opt_i64", "gt", 500_000_000), E]},
    "not_contains beside is_null": {"or": [L("message", "not_contains", "e"), E]},
    "not_contains beside a term true on null rows": {"or": [
        L("message", "not_icontains", "r"), L("latency", "lt", 200_000)]},
    "empty literal": {"or": [L("message", "contains", ""),
                             L("latency", "lt", 100_000)]},
    "negated empty literal": {"or": [L("message", "not_contains", ""),
                                     L("level", "eq", "ERROR")]},
    "folded group inside a general one": {"or": [
        L("opt_i64", "is_null"),
        {"and": [Cc, {"or": [L("level", "eq", "INFO"), L("level", "eq", "Info"),
                             L("level", "ends_with", "N")]}]}]},
    "null-bearing f64 under or": {"or": [
        L("f_f64", "lt", 0.1), {"and": [L("f_f64", "is_null"), A]},
        {"and": [L("f_f64", "ge", 0.95), F]}]},
    "root preds and time range": {"or": [B, {"and": [A, D]}]},
}


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(c6, session, capfd, name):
    q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"}],
         "group_by": ["level"], "where": SHAPES[name]}
    if name == "root preds and time range":
        q["preds"] = [L("latency", "ne", 7), L("tag", "is_not_null")]
        q["time_range"] = [BASE + 30_000, BASE + 2 * MIN + 10_000]
    _, err = _check(c6, session, q, capfd)
    assert "[gpuq plan] where " in err
    if name == "depth 3":
        assert re.search(r"contexts=7 depth=3", err), err[-1500:]
        assert re.search(r"where bufs=6 combines=6", err), err[-1500:]
    if name == "five terms":
        assert re.search(r"or node=\d+ terms=5 path=mask", err)
        assert re.search(r"where bufs=2 combines=5", err), err[-1500:]
    if name == "folded group inside a general one":
        assert sorted(_or_paths(err)) == ["lut", "mask"]
    if name.startswith("not_contains beside"):
        # a NULL message fails the negated leaf: those rows are selected
        # through the other term alone — all of them beside is_null, some
        # beside the latency leaf
        data = c6["data"]
        sel = set(wc.selected(data, q))
        nulls = {i for i, v in enumerate(data["message"]) if v is None}
        if name.endswith("is_null"):
            assert nulls <= sel
        else:
            assert sel & nulls and nulls - sel


# ---- consumers of the mask --------------------------------------------------------

TREE = {"or": [B, {"and": [Cc, {"or": [D, E]}]}]}


def test_group_by_aggregates(c6, session, capfd):
    q = {"select": [{"agg": "count_star"}, {"agg": "sum", "col": "latency"},
                    {"agg": "min", "col": "opt_i64"},
                    {"agg": "max", "col": "opt_i64"},
                    {"agg": "avg", "col": "latency"},
                    {"agg": "count", "col": "message"}],
         "group_by": ["level"], "where": TREE}
    _check(c6, session, q, capfd)


def test_count_distinct(c6, session, capfd):
    q = {"select": [{"agg": "count_distinct", "col": "level"},
                    {"agg": "count_distinct", "col": "opt_i64"},
                    {"agg": "count_star"}], "where": TREE}
    _check(c6, session, q, capfd)
    q = {"select": [{"agg": "count_distinct", "col": "tag"}],
         "group_by": ["level"], "where": TREE}
    _check(c6, session, q, capfd)


@pytest.mark.parametrize("limit", [50, None])
def test_projection(c6, session, capfd, limit):
    q = {"select_cols": ["p_timestamp", "level", "latency"], "where": TREE}
    if limit:
        q["limit"] = limit
    data = c6["data"]
    want_all = wc.expected(data, dict(q, limit=None))
    assert 50 < len(want_all) < len(data["p_timestamp"])
    rows, _ = _gpu(c6, session, q, capfd)
    if limit:
        assert want_all[limit - 1][0] != want_all[limit][0]   # no tie on the cut
    want = want_all[:limit] if limit else want_all
    assert [r[0] for r in rows] == [r[0] for r in want]
    canon = lambda rs: sorted(rs, key=lambda r: (-r[0], str(r[1]), r[2]))
    assert canon(rows) == canon(want)


def test_fused_value_aggregate(c6, session, capfd):
    """The fused shape (one key, count(*) + one i64 aggregate over a column
    nothing else reads) keeps its path under an OR: the mask is final before
    k_val_agg runs."""
    for agg in ("sum", "min", "max"):
        q = {"select": [{"agg": "count_star"}, {"agg": agg, "col": "latency"}],
             "group_by": ["level"], "where": {"or": [B, D, E]}}
        _, err = _check(c6, session, q, capfd)
        assert re.search(r"fused_valagg=1", err), err[-1500:]
        assert re.findall(r"\[gpuq exec\] part \d+: valagg=(\w+)", err) == ["fused"]
        assert re.search(r"where bufs=2 combines=3", err), err[-1500:]


@pytest.mark.parametrize("name", ["(A or B) and (C or D)", "depth 3",
                                  "same column and op in two contexts",
                                  "null-bearing column under or"])
def test_rows_no_multiple_of_16(c6_odd, session, capfd, name):
    data = c6_odd["data"]
    assert len(data["p_timestamp"]) == 1003
    q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"}],
         "group_by": ["level"], "where": SHAPES[name]}
    _check(c6_odd, session, q, capfd)
    q = {"select": COUNT, "where": SHAPES[name],
         "time_range": [BASE + 7_000, BASE + 2 * MIN + 3_000]}
    _check(c6_odd, session, q, capfd)


@pytest.mark.parametrize("name", list(SHAPES))
def test_planners_agree(c6, session, capfd, name):
    q = {"select": [{"agg": "count_star"}, {"agg": "min", "col": "opt_i64"}],
         "group_by": ["level"], "where": SHAPES[name],
         "time_range": [BASE + 20_000, BASE + 2 * MIN + 40_000]}
    a, err_a = _check(c6, session, q, capfd)
    b, err_b = _check(c6, session, q, capfd, py_planner=True)
    assert a == b
    pick = lambda e: re.findall(r"\[gpuq (?:plan\] (?:where|or) |exec\] part \d+: where).*", e)
    assert pick(err_a) == pick(err_b) and pick(err_a)


# ---- seeded random trees ---------------------------------------------------------

@pytest.fixture(scope="module")
def trees(c6):
    return wc.random_trees(c6["data"])


@pytest.mark.parametrize("chunk", range(6))
def test_random_trees(c6, session, capfd, trees, chunk):
    from oracle.compare import assert_rows_equal

    data = c6["data"]
    assert len(trees) >= 40
    part = trees[chunk::6]
    assert part
    for t, n_sel in part:
        q = wc.query_for(t)
        rows, err = _gpu(c6, session, q, capfd)
        want = wc.expected(data, q)
        assert sum(r[-1] for r in want) == n_sel
        assert_rows_equal(rows, want, f"GPU vs python: {t}")
