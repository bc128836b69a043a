"""Device page decoders against the page-case fixtures
(tests/pagecases_common.py; tests/test_pagecases_cpu.py proves each file
holds the page shapes named below).

Every expected value comes from the source arrays the files were written
from, through pc.ref_query (plain Python, exact ints); where the pyarrow
oracle evaluates a query exactly it is run as a second opinion. All
comparisons are exact: ints and strings by ==, doubles by bit pattern.
Columns whose sum can overflow int64 are only counted, projected, grouped
and min/max-ed.

Device errors: a kernel that reports ERR_DELTA, ERR_DICT_RANGE, ... makes
gpuq_plan_execute fail, which GpuExecutionPlan raises as GpuqError — every
query here goes through _run, so a swallowed error code fails the test.

Decoder entry points and what reaches them:
  k_delta_i64 fast path      projection / lt,ge / min,max of d_*_req, d_*_nn
  k_delta_i64 serial path    the same over d_*_nul (nulls), i32_delta_nul
  k_plain_fixed mode 2       i64_plain/f64_plain/i32_plain _req, _nn (footer
                             null-free), mode 0 + 1: _nul and i_<layout>
                             (mode 0 takes the all-valid pages of a
                             null-bearing chunk: def_mp i_runs, i_null_first)
  dict_page_decode generic   EmitGid / EmitDictI64 / EmitDictMask / EmitLutD:
                             group by x_str_*, projection of x_*, eq/ne on
                             x_str_* — modes 2 (_req, _nn), 0 and 1 (_nul, mp)
  dict_page_decode batched   k_val_agg over x_i64_* _req/_nn (mode 2 only:
                             the fused path requires a null-free column)
  k_dict_count fast, serial  GROUP BY x_str_D + count(*) without predicate,
                             D <= 4097: _req/_nn fast, _nul/mp SerialRle
  k_val_agg                  min/max of x_i64_*, i64_plain_* by k (PLAIN and
                             dictionary branches), against k_dict_i64 /
                             k_plain_fixed under GPUQ_NO_FUSED_VALAGG=1
  k_def_levels               every _nul column and every def layout
  k_expand modes 0, 1, 2     projection of _nul values, GROUP BY a null-
                             bearing x_str_*, eq/ne on a null-bearing x_str_*

The snappy / uncompressed twins get one query each: their whole-file
projection.

INT32 DELTA_BINARY_PACKED is decoded (not refused): k_delta_i64 sums in
wrapping 64-bit arithmetic and narrows each value to 32 bits with sign
extension at the store, which equals the writer's 32-bit wrapping sums.

Not reachable from pyarrow-written files, so not covered here: dictionary
index width 0 with values present, and a null-free page whose def levels are
two RLE runs (the all_valid probe's negative case on a footer-proven
null-free column); see tests/test_pagecases_cpu.py.
"""

import os
import re

import pytest

from tests import pagecases_common as pc

pytestmark = pytest.mark.gpu

# A query costs about a third of a second whatever the file size (plan
# build, load, execute), so the module is sized by its query count: whole
# files per projection, up to MAX_AGGS aggregates per old-path query, one
# query per decoder path and index width where the path admits one column.
PROJ_CHUNK = 64     # columns per projection query: every file in one


@pytest.fixture(scope="module")
def cs(tmp_path_factory):
    return pc.CaseSet(tmp_path_factory.mktemp("pagecases_gpu"))


@pytest.fixture(scope="module")
def session():
    from parseable_amd import GpuSession

    return GpuSession()


def _run(session, case, q, env=None, capfd=None):
    """Rows of q over the single file of case; with capfd also the plan /
    exec debug lines. Raises on a plan-build error and on any device error."""
    from parseable_amd.provider import GpuExecutionPlan, merge_partials

    env = dict(env or {})
    if capfd is not None:
        env["GPUQ_PLAN_DEBUG"] = "1"
        capfd.readouterr()
    os.environ.update(env)
    try:
        plan = GpuExecutionPlan(session, [case.path], dict(q))
        try:
            if plan.empty:       # footers prove that no row can match
                rows = [] if q.get("select_cols") else merge_partials([], q)
            else:
                plan.load()
                rows = plan.execute_all()
        finally:
            plan.close()
    finally:
        for k in env:
            os.environ.pop(k, None)
    if capfd is None:
        return rows
    return rows, capfd.readouterr().err


def _assert_rows(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} rows, want {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        bad = pc.first_mismatch(g, w)
        assert bad is None, f"{what}: result row {i} ({g!r} vs {w!r}): {bad}"


_ORACLE_EXACT_AGGS = ("count_star", "count")


def _check(session, case, q, what, env=None, capfd=None, oracle=None):
    """GPU == ref_query over the source arrays; and == the pyarrow oracle
    where that is exact. The oracle reads null-bearing int columns through
    float64, so by default it is consulted for counts only."""
    from oracle import query_oracle as qo

    out = _run(session, case, q, env, capfd)
    rows = out[0] if capfd is not None else out
    _assert_rows(rows, pc.ref_query(case, q), f"{what} vs source arrays")
    if oracle is None:
        oracle = (not q.get("select_cols") and all(
            a["agg"] in _ORACLE_EXACT_AGGS for a in q["select"]) and all(
            p["op"] not in ("is_null", "is_not_null")
            for p in q.get("preds", [])))
    if oracle:
        _assert_rows(rows, qo.execute([case.path], dict(q))["rows"],
                     f"{what} vs oracle")
    return out


# ---------------------------------------------------------------------------
# full projection of every column of every file: exact decoded values
# ---------------------------------------------------------------------------

def _data_cols(name):
    """Column names of a case without building it."""
    if name.startswith("delta_ts"):
        return ["k", "o", "v"]
    if name.startswith("delta"):
        stems = [f"d_{b}" for b in pc.DELTA_WIDTHS + pc.DELTA_EXTRA]
        return ["k", "o"] + [f"{s}_{v}" for s in stems for v in pc.VARIANTS]
    if name.startswith("dict"):
        sizes = pc.DICT_SIZES_SMALL if "small" in name else pc.DICT_SIZES_BIG
        return ["k", "o"] + [f"x_{t}_{d}" for d in sizes for t in pc.DICT_TYPES]
    if name.startswith("def"):
        return ["k", "o"] + [f"{p}_{l}" for l in pc.DEF_LAYOUTS
                             for p in ("i", "s")]
    if name == "int32":
        stems = [f"i32_{k}" for k in pc.INT32_KINDS] + ["i64_plain", "f64_plain"]
        return ["k", "o"] + [f"{s}_{v}" for s in stems for v in pc.VARIANTS]
    assert name == "int32_ovf"
    return ["k", "o"] + [f"i32_ovf_{v}" for v in pc.VARIANTS]


PROJ_PARAMS = [(n, c) for n in pc.CASE_NAMES for c in _data_cols(n)]
_proj = {}


def _projection(session, case, col):
    """Result column `col` of the full projection, one query per chunk of
    PROJ_CHUNK columns, each run once."""
    cols = _data_cols(case.name)
    assert ["p_timestamp"] + cols == list(case.cols)
    ci = cols.index(col) // PROJ_CHUNK
    key = (case.name, ci)
    if key not in _proj:
        chunk = cols[ci * PROJ_CHUNK:(ci + 1) * PROJ_CHUNK]
        q = {"select_cols": ["p_timestamp"] + chunk, "limit": case.n}
        try:
            _proj[key] = (q, _run(session, case, q))
        except Exception as e:          # every column of the chunk reports it
            _proj[key] = (q, e)
    q, rows = _proj[key]
    if isinstance(rows, Exception):
        raise rows
    j = q["select_cols"].index(col)
    return [r[0] for r in rows], [r[j] for r in rows]


@pytest.mark.parametrize("name,col", PROJ_PARAMS,
                         ids=[f"{n}-{c}" for n, c in PROJ_PARAMS])
def test_projection_all_rows(cs, session, name, col):
    """SELECT p_timestamp, col ... LIMIT n_rows: every row, element by
    element including null positions."""
    case = cs.case(name)
    ts, got = _projection(session, case, col)
    order = sorted(range(case.n), key=lambda i: -case.cols["p_timestamp"][i])
    assert ts == [case.cols["p_timestamp"][i] for i in order]
    bad = pc.first_mismatch(got, [case.cols[col][i] for i in order])
    assert bad is None, f"{name}.{col}: {bad}"


def test_projection_unlimited_reader(cs, session):
    """The streamed (unlimited) projection path over the multi-page delta
    file, widths 59-63 with and without nulls."""
    case = cs.case(f"delta_mp_{pc.DELTA_MP_ROWS}")
    cols = [f"d_{b}_{v}" for b in pc.DELTA_HARD_WIDTHS for v in ("nn", "nul")]
    q = {"select_cols": ["p_timestamp"] + cols}
    _check(session, case, q, "unlimited projection")


def test_projection_delta_timestamp(cs, session):
    """p_timestamp itself delta-encoded and shuffled by hours: rows come
    back in timestamp order carrying their own row index."""
    case = cs.case("delta_ts")
    ts, v = _projection(session, case, "v")
    assert ts == sorted(case.cols["p_timestamp"], reverse=True)
    assert sorted(v) == list(range(case.n)) and v != sorted(v)
    q = {"select": [{"agg": "count_star"}, {"agg": "min", "col": "p_timestamp"},
                    {"agg": "max", "col": "p_timestamp"}], "group_by": ["k"]}
    _check(session, case, q, "delta_ts min/max", oracle=True)


# ---------------------------------------------------------------------------
# dictionary index decoders
# ---------------------------------------------------------------------------

# one dictionary size per index bit width, plus the sizes either side of a
# width change: widths 1, 1, 2, 3, 4, 8, 9, 10, 12, 13 (16, 17 in the big files)
WIDTH_SIZES = (1, 2, 4, 5, 9, 256, 257, 513, 4095, 4097)

FUSED_COUNT = ([("dict_small_req" if i % 2 else "dict_small_nn", d, "fast")
                for i, d in enumerate(WIDTH_SIZES)]
               + [("dict_small_mp", d, "serial") for d in (2, 257, 4097)]
               + [("dict_small_nul", d, "serial") for d in (1, 9, 4095)])


@pytest.mark.parametrize("name,d,path", FUSED_COUNT,
                         ids=[f"{n}-x_str_{d}-{p}" for n, d, p in FUSED_COUNT])
def test_group_by_utf8_fused_count(cs, session, capfd, name, d, path):
    """GROUP BY x_str_D + count(*), no predicate: k_dict_count — the wave-
    parallel unpack on all-valid pages (_req without def levels, _nn behind
    the all-valid probe), lane 0's SerialRle pair on null-bearing pages."""
    case = cs.case(name)
    col = f"x_str_{d}"
    q = {"select": [{"agg": "count_star"}], "group_by": [col]}
    _, err = _check(session, case, q, f"{name} {col} k_dict_count {path}",
                    capfd=capfd)
    assert "[gpuq plan] fused_count=1" in err, err[-2000:]


DICT_GID = [("dict_small_req", 4), ("dict_small_req", 257),
            ("dict_small_nn", 4097), ("dict_small_mp", 5),
            ("dict_small_mp", 513), ("dict_small_nul", 4095),
            ("dict_big_nn", 65537), ("dict_big_nul", 65535),
            ("dict_big_mp", 65537)]


@pytest.mark.parametrize("name,d", DICT_GID,
                         ids=[f"{n}-x_str_{d}" for n, d in DICT_GID])
def test_group_by_utf8_dict_gid(cs, session, capfd, name, d):
    """The same key with a predicate and a second aggregate: k_dict_gid in
    mode 2 (_req, _nn) or modes 0 + 1 with k_expand mode 1 (nulls). The big
    dictionaries exceed the fused histogram with or without a predicate."""
    case = cs.case(name)
    col = f"x_str_{d}"
    q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "o"}],
         "group_by": [col], "preds": [{"col": "o", "op": "ge", "lit": -500}]}
    _, err = _check(session, case, q, f"{name} {col} k_dict_gid", capfd=capfd,
                    oracle=True)      # o has no nulls: the oracle is exact
    assert "[gpuq plan] fused_count=0" in err


DICT_NUM_KEY = [("dict_small_nul", "i64", 257), ("dict_small_req", "f64", 4097),
                ("dict_small_nn", "f64", 5), ("dict_big_mp", "i64", 65537)]


@pytest.mark.parametrize("name,typ,d", DICT_NUM_KEY,
                         ids=[f"{n}-x_{t}_{d}" for n, t, d in DICT_NUM_KEY])
def test_group_by_numeric_dict(cs, session, name, typ, d):
    """GROUP BY a numeric dictionary column: k_dict_i64 + numeric hash."""
    case = cs.case(name)
    q = {"select": [{"agg": "count_star"}], "group_by": [f"x_{typ}_{d}"]}
    _check(session, case, q, f"{name} x_{typ}_{d} numeric key")


DICT_PRED = [("dict_small_nn", 2, "eq"), ("dict_small_req", 257, "eq"),
             ("dict_small_nn", 4097, "ne"), ("dict_small_mp", 2, "ne"),
             ("dict_small_nul", 257, "ne"), ("dict_small_mp", 4097, "eq"),
             ("dict_big_nul", 65537, "eq"), ("dict_big_req", 65535, "ne")]


@pytest.mark.parametrize("name,d,op", DICT_PRED,
                         ids=[f"{n}-x_str_{d}-{o}" for n, d, o in DICT_PRED])
def test_eq_ne_on_utf8_dict(cs, session, name, d, op):
    """Literal from the dictionary: k_dict_mask (direct), and k_dict_lut_scr
    + k_expand mode 2 on null-bearing pages."""
    case = cs.case(name)
    lit = pc.dict_value("str", d // 2)
    q = {"select": [{"agg": "count_star"}, {"agg": "count", "col": "o"}],
         "preds": [{"col": f"x_str_{d}", "op": op, "lit": lit}]}
    rows = _check(session, case, q, f"{name} x_str_{d} {op} {lit!r}")
    assert 0 < rows[0][0] < case.n


@pytest.mark.parametrize("typ", pc.DICT_TYPES)
@pytest.mark.parametrize("name", ["dict_small_req", "dict_small_mp"])
def test_ne_on_every_dict_width(cs, session, name, typ):
    """x_D != entry for many D at once: one mask decode per column (LUT
    mask for utf8, value decode + compare for numbers) in one conjunction.
    A row survives unless one of its values is the literal or NULL, so the
    null-bearing file takes D >= 9 only: enough rows survive there for a
    wrong mask in any one column to change the count."""
    case = cs.case(name)
    preds = [{"col": f"x_{typ}_{d}", "op": "ne",
              "lit": pc.dict_value(typ, d // 2)}
             for d in pc.DICT_SIZES_SMALL
             if d >= (2 if name.endswith("_req") else 9)]
    q = {"select": [{"agg": "count_star"}], "preds": preds}
    rows = _check(session, case, q, f"{name} x_{typ}_* ne")
    assert 0 < rows[0][0] < case.n


# ---------------------------------------------------------------------------
# min / max / sum by a small key: k_val_agg against the materialising kernels
# ---------------------------------------------------------------------------

def _plan_path(err):
    m = re.search(r"\[gpuq plan\] fused_count=\d fused_valagg=(\d)", err)
    assert m, "no plan debug line on fd 2:\n" + err[-2000:]
    execs = set(re.findall(r"\[gpuq exec\] part \d+: valagg=(\w+)", err))
    return "old" if m.group(1) == "0" else "+".join(sorted(execs))


def _aggs_by_k(session, case, pairs, capfd, env=None):
    """count(*) and up to 7 (agg, col) aggregates GROUP BY k in one query:
    more than two aggregates keep the plan on the materialising path."""
    assert len(pairs) <= 7
    q = {"select": [{"agg": "count_star"}]
         + [{"agg": a, "col": c} for a, c in pairs], "group_by": ["k"]}
    nonnull = all(v is not None for _, c in pairs for v in case.cols[c])
    return _check(session, case, q, f"{case.name} {pairs}", env=env,
                  capfd=capfd, oracle=nonnull)


VALAGG_FUSED = ([("dict_small_req" if i % 2 else "dict_small_nn", f"x_i64_{d}",
                  "max" if i % 2 else "min")
                 for i, d in enumerate((2, 5, 9, 257, 513, 4097))]
                + [("dict_big_nn", "x_i64_65535", "max"),
                   ("dict_big_req", "x_i64_65537", "min"),
                   ("int32", "i64_plain_req", "max"),
                   ("int32", "i64_plain_nn", "min")])


@pytest.mark.parametrize("name,col,agg", VALAGG_FUSED,
                         ids=[f"{n}-{a}-{c}" for n, c, a in VALAGG_FUSED])
def test_valagg_fused(cs, session, capfd, name, col, agg):
    """count(*) + min|max of a null-free INT64 column by k takes k_val_agg:
    the batched dict_page_decode for dictionary pages, the PLAIN branch for
    i64_plain. GPUQ_NO_FUSED_VALAGG=1 must give the same rows through
    k_dict_i64 / k_plain_fixed."""
    case = cs.case(name)
    rows, err = _aggs_by_k(session, case, [(agg, col)], capfd)
    assert _plan_path(err) == "fused", err[-2000:]
    old, err = _aggs_by_k(session, case, [(agg, col)], capfd,
                          env={"GPUQ_NO_FUSED_VALAGG": "1"})
    assert _plan_path(err) == "old"
    _assert_rows(old, rows, "GPUQ_NO_FUSED_VALAGG=1 vs fused")


def _chunks(pairs, n=7):
    return [pairs[i:i + n] for i in range(0, len(pairs), n)]


OLD_PATH = (
    # null-bearing dictionary INT64: k_dict_i64 modes 0 + 1, k_expand mode 0
    [("dict_small_nul", c) for c in _chunks(
        [("min" if d % 2 else "max", f"x_i64_{d}") for d in WIDTH_SIZES])]
    + [("dict_small_mp", c) for c in _chunks(
        [("max" if d % 2 else "min", f"x_i64_{d}") for d in WIDTH_SIZES])]
    + [("dict_big_mp", [("min", "x_i64_65535"), ("max", "x_i64_65537")])]
    # INT32 in every encoding, widened by the decoders; 3,000 values below
    # 2**31 cannot overflow an int64 sum
    + [("int32", [(a, f"i32_{k}_{v}") for v in pc.VARIANTS
                  for a in ("min", "max")]) for k in pc.INT32_KINDS]
    + [("int32", [("sum", f"i32_{k}_{v}") for k in pc.INT32_KINDS
                  for v in ("req", "nul")])]
    + [("int32_ovf", [(a, f"i32_ovf_{v}") for v in pc.VARIANTS
                      for a in ("min", "max")])]
    + [("int32_ovf", [("sum", f"i32_ovf_{v}") for v in pc.VARIANTS])]
    # delta pages (fast and serial path), the spilling widths first
    + [("delta_1000", c) for c in _chunks(
        [("max", f"d_{b}_{v}") for b in pc.DELTA_HARD_WIDTHS
         for v in pc.VARIANTS]
        + [("min", f"d_64_{v}") for v in pc.VARIANTS]
        + [("min", "d_alt_nul"), ("max", "d_1_nul"), ("min", "d_33_req")])]
    # PLAIN DOUBLE and null-bearing PLAIN INT64 (k_plain_fixed modes 0 + 1)
    + [("int32", [(a, f"f64_plain_{v}") for v in pc.VARIANTS
                  for a in ("min", "max")] + [("max", "i64_plain_nul")])]
)


@pytest.mark.parametrize("name,pairs", OLD_PATH,
                         ids=[f"{n}-{p[0][1]}..{p[-1][1]}" for n, p in OLD_PATH])
def test_aggregates_materialising_path(cs, session, capfd, name, pairs):
    _, err = _aggs_by_k(session, cs.case(name), pairs, capfd)
    assert _plan_path(err) == "old"


# ---------------------------------------------------------------------------
# comparisons on delta / INT32 columns, counts on the def layouts
# ---------------------------------------------------------------------------

def _quantile(case, col, f):
    vals = sorted(v for v in case.cols[col] if v is not None)
    return vals[int(len(vals) * f)]


CMP = [
    ("delta_1000", "ge", [f"d_{b}_req" for b in pc.DELTA_HARD_WIDTHS]),
    ("delta_1000", "lt", [f"d_{b}_nul" for b in pc.DELTA_HARD_WIDTHS]),
    ("delta_1000", "ge", ["d_1_nn", "d_32_nul", "d_64_nn", "d_dec_req"]),
    (f"delta_mp_{pc.DELTA_MP_ROWS}", "ge",
     [f"d_{b}_nul" for b in pc.DELTA_HARD_WIDTHS]),
    ("int32", "lt", [f"i32_{k}_nul" for k in pc.INT32_KINDS]),
    ("int32", "ge", [f"i32_{k}_req" for k in pc.INT32_KINDS]),
    ("int32_ovf", "lt", ["i32_ovf_nn", "i32_ovf_nul"]),
]


@pytest.mark.parametrize("name,op,cols", CMP,
                         ids=[f"{n}-{o}-{c[0]}..{c[-1]}" for n, o, c in CMP])
def test_lt_ge_on_delta_and_int32(cs, session, name, op, cols):
    """col >= its 10 % quantile (col < its 90 % quantile) for several
    columns at once: k_cmp_i64 over each decoded column; count(col) of the
    first rides along."""
    case = cs.case(name)
    f = 0.1 if op == "ge" else 0.9
    q = {"select": [{"agg": "count_star"}, {"agg": "count", "col": cols[0]}],
         "preds": [{"col": c, "op": op, "lit": _quantile(case, c, f)}
                   for c in cols]}
    rows = _check(session, case, q, f"{name} {cols} {op}")
    assert 0 < rows[0][0] < case.n


@pytest.mark.parametrize("name", ["def", "def_mp"])
@pytest.mark.parametrize("pre", ["i", "s"])
def test_def_level_count_col(cs, session, name, pre):
    """count(col) under every null layout at once: k_def_levels' run walk
    (bit-packed groups at unaligned positions, RLE runs across 64-row words)
    counted against the source arrays."""
    case = cs.case(name)
    cols = [f"{pre}_{l}" for l in pc.DEF_LAYOUTS]
    q = {"select": [{"agg": "count_star"}]
         + [{"agg": "count", "col": c} for c in cols], "group_by": ["k"]}
    rows = _check(session, case, q, f"{name} count({pre}_*)")
    for j, c in enumerate(cols):
        assert sum(r[2 + j] for r in rows) == sum(
            v is not None for v in case.cols[c]), c


NULL_PRED = [("def", "i_runs", "is_null"), ("def", "s_runs", "is_not_null"),
             ("def", "s_null_first", "is_null"),
             ("def", "i_null_last", "is_not_null"),
             ("def", "i_all_valid", "is_null"),
             ("def_mp", "s_runs", "is_null"), ("def_mp", "i_alt", "is_not_null"),
             ("def_mp", "i_all_null", "is_not_null")]


@pytest.mark.parametrize("name,col,op", NULL_PRED,
                         ids=[f"{n}-{c}-{o}" for n, c, o in NULL_PRED])
def test_is_null_predicates(cs, session, name, col, op):
    case = cs.case(name)
    n_valid = sum(v is not None for v in case.cols[col])
    q = {"select": [{"agg": "count_star"}, {"agg": "count", "col": col}],
         "preds": [{"col": col, "op": op}]}
    rows = _check(session, case, q, f"{name} {col} {op}")
    assert rows[0][0] == (n_valid if op == "is_not_null" else case.n - n_valid)


@pytest.mark.parametrize("name,col", [("int32", "i32_delta_nul"),
                                      ("int32", "i32_plain_req"),
                                      ("delta_1000", "d_63_nul")])
def test_count_distinct(cs, session, name, col):
    """The distinct-set pass over decoded values. i32_delta_nul repeats its
    first 200 values (two extremes), so a mis-decode changes the count; the
    random columns are all-distinct and pin the path, not the values (the
    projection test pins those)."""
    case = cs.case(name)
    q = {"select": [{"agg": "count_star"}, {"agg": "count_distinct", "col": col}],
         "group_by": ["k"]}
    _check(session, case, q, f"{name} count_distinct({col})")


@pytest.mark.parametrize("name,col", [("int32", "i32_delta_nul"),
                                      ("int32_ovf", "i32_ovf_req"),
                                      ("delta_257", "d_62_nul")])
def test_group_by_numeric_value_column(cs, session, name, col):
    """A PLAIN / delta column as the group key: numeric hash over the
    decoded values, NULL group included."""
    case = cs.case(name)
    q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "o"}],
         "group_by": [col]}
    _check(session, case, q, f"{name} group by {col}")


# ---------------------------------------------------------------------------
# out of scope for the decoders: refused at plan build, never mis-decoded
# ---------------------------------------------------------------------------

REFUSED = [("unsupported_types_case", "b", "unsupported column type BOOLEAN"),
           ("unsupported_types_case", "f", "unsupported column type FLOAT"),
           ("unsupported_types_case", "x",
            "unsupported column type FIXED_LEN_BYTE_ARRAY"),
           ("int96_case", "t96", "unsupported column type INT96"),
           ("page_v2_case", "v", "data page v2")]


@pytest.mark.parametrize("shape", ["projection", "min", "count", "group_by"])
@pytest.mark.parametrize("builder,col,text", REFUSED,
                         ids=[t.split()[-1] for _, _, t in REFUSED])
def test_refused_at_plan_build(tmp_path_factory, session, builder, col, text,
                               shape):
    """BOOLEAN, FLOAT, INT96, FIXED_LEN_BYTE_ARRAY columns and v2 data pages
    have no decoder: building a plan that reads one fails with a message
    naming the reason, before any kernel runs."""
    from parseable_amd.provider import GpuExecutionPlan, GpuqError

    path = getattr(pc, builder)(str(tmp_path_factory.mktemp("refused")))
    q = {"projection": {"select_cols": ["p_timestamp", col], "limit": 10},
         "min": {"select": [{"agg": "min", "col": col}]},
         "count": {"select": [{"agg": "count_star"},
                              {"agg": "count", "col": col}]},
         "group_by": {"select": [{"agg": "count_star"}], "group_by": [col]},
         }[shape]
    if shape == "group_by" and "v2" not in text:
        text = "unsupported group-key type"     # the key check comes first
    with pytest.raises(GpuqError, match=text):
        GpuExecutionPlan(session, [path], q)
