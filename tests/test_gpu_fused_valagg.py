"""Fused value-decode + aggregate (k_val_agg) and the footer-proven
null-free single-launch decode mode.

Every case is checked three ways: exactly against the oracle, exactly
against the same query with GPUQ_NO_FUSED_VALAGG=1 (the materialise-then-
aggregate kernels), and for the path it took, read from the GPUQ_PLAN_DEBUG
lines the library writes to fd 2:
  [gpuq plan] fused_count=. fused_valagg=0|1 ...     (plan build)
  [gpuq exec] part N: valagg=fused|fallback ...      (each execute)

Data: c1, 600,000 rows in 262,144-row files — two full files whose latency
and f_i64 chunks overflow the dictionary (dict pages followed by PLAIN
pages) plus one 75,712-row file whose latency chunk is dict only. f_i64
holds negative values (signed min/max init, wrap-free sums)."""

import os
import re

import pytest

pytestmark = pytest.mark.gpu

BASE = 1756684800000
MIN = 60_000


@pytest.fixture(scope="module")
def c1(tmp_path_factory):
    from datagen.gen import gen_stream

    td = tmp_path_factory.mktemp("valagg_c1")
    return gen_stream(str(td), "s", "c1", rows=600_000, rows_per_file=262_144)


@pytest.fixture(scope="module")
def c4(tmp_path_factory):
    from datagen.gen import gen_stream

    td = tmp_path_factory.mktemp("valagg_c4")
    return gen_stream(str(td), "s", "c4", rows=100_000)


@pytest.fixture(scope="module")
def c5(tmp_path_factory):
    from datagen.gen import gen_stream

    td = tmp_path_factory.mktemp("valagg_c5")
    return gen_stream(str(td), "s", "c5", rows=100_000)


@pytest.fixture(scope="module")
def c1_small(tmp_path_factory):
    from datagen.gen import gen_stream

    td = tmp_path_factory.mktemp("valagg_c1s")
    return gen_stream(str(td), "s", "c1", rows=100_000)


@pytest.fixture(scope="module")
def session():
    from parseable_amd import GpuSession

    return GpuSession()


_ORACLE = {}


def _oracle(info, q):
    """Oracle rows, computed once per (stream, query) and shared."""
    import json

    from oracle import query_oracle as qo

    key = (info["stream_dir"], json.dumps(q, sort_keys=True))
    if key not in _ORACLE:
        _ORACLE[key] = qo.execute(info["files"], dict(q))["rows"]
    return _ORACLE[key]


def _gpu(info, session, q, capfd, no_fused):
    """Run q with plan debugging on; return (rows, path) where path is
    'fused', 'fallback' (eligible plan, too many groups at execute) or 'old'
    (plan not eligible)."""
    from parseable_amd import Query, StandardTableProvider

    os.environ["GPUQ_PLAN_DEBUG"] = "1"
    if no_fused:
        os.environ["GPUQ_NO_FUSED_VALAGG"] = "1"
    try:
        capfd.readouterr()
        prov = StandardTableProvider(info["stream_dir"], session)
        rows, _ = Query(prov).execute(dict(q))
        err = capfd.readouterr().err
    finally:
        os.environ.pop("GPUQ_PLAN_DEBUG", None)
        os.environ.pop("GPUQ_NO_FUSED_VALAGG", None)
    m = re.search(r"\[gpuq plan\] fused_count=\d fused_valagg=(\d)", err)
    assert m, "no plan debug line on fd 2:\n" + err[-2000:]
    execs = re.findall(r"\[gpuq exec\] part \d+: valagg=(\w+)", err)
    if m.group(1) == "0":
        assert not execs
        return rows, "old"
    assert execs and len(set(execs)) == 1, execs
    return rows, execs[0]


def _check(info, session, q, capfd, want_path):
    from oracle.compare import assert_rows_equal

    rows, path = _gpu(info, session, q, capfd, no_fused=False)
    assert path == want_path, f"path {path}, expected {want_path}: {q}"
    old_rows, old_path = _gpu(info, session, q, capfd, no_fused=True)
    assert old_path == "old"
    assert_rows_equal(rows, _oracle(info, q), "GPU vs oracle")
    assert_rows_equal(rows, old_rows, "fused vs GPUQ_NO_FUSED_VALAGG=1")
    return rows


# whole files 0 and 1 (timestamps of file f lie in [BASE + f*MIN, +MIN)):
# chunk statistics prove the predicate, no selection mask is built
WHOLE = {"col": "p_timestamp", "op": "between", "lo": BASE,
         "hi": BASE + 2 * MIN - 1}
# bounds inside files 0 and 1: boundary row groups, masked rows
INSIDE = {"col": "p_timestamp", "op": "between", "lo": BASE + MIN // 2,
          "hi": BASE + MIN + MIN // 3}


@pytest.mark.parametrize("pred", [None, WHOLE, INSIDE],
                         ids=["nopred", "whole_files", "inside_file"])
@pytest.mark.parametrize("col", ["latency", "f_i64"])
@pytest.mark.parametrize("agg", ["max", "min", "sum"])
def test_fused_group_by_host(c1, session, capfd, agg, col, pred):
    q = {"select": [{"agg": "count_star"}, {"agg": agg, "col": col}],
         "group_by": ["host"]}
    if pred:
        q["preds"] = [dict(pred)]
    rows = _check(c1, session, q, capfd, "fused")
    if pred is None:
        assert sum(r[1] for r in rows) == 600_000
    if pred is WHOLE:
        assert sum(r[1] for r in rows) == 2 * 262_144
    if pred is INSIDE:
        assert 0 < sum(r[1] for r in rows) < 2 * 262_144


@pytest.mark.parametrize("key", ["level", "f_str1"])
def test_fused_other_keys(c1, session, capfd, key):
    q = {"select": [{"agg": "count_star"}, {"agg": "min", "col": "f_i64"}],
         "group_by": [key], "preds": [dict(INSIDE)]}
    _check(c1, session, q, capfd, "fused")


def test_fused_hash_key_checked_at_execute(c5, session, capfd):
    """A raw-byte utf8 key (PLAIN-fallback pages, device hash gids): the
    group count is known only at execute; 1,500 groups fit the LDS table."""
    q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"}],
         "group_by": ["trace"]}
    _check(c5, session, q, capfd, "fused")


def test_old_path_compare_pred_on_agg_column(c1, session, capfd):
    q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"}],
         "group_by": ["host"],
         "preds": [{"col": "latency", "op": "ge", "lit": 500_000}]}
    _check(c1, session, q, capfd, "old")


def test_old_path_delta_encoded_column(c1, session, capfd):
    q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "p_timestamp"}],
         "group_by": ["host"]}
    _check(c1, session, q, capfd, "old")


def test_old_path_null_bearing_agg_column(c4, session, capfd):
    q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "attr_i0"}],
         "group_by": ["service"]}
    _check(c4, session, q, capfd, "old")


def test_fallback_more_groups_than_lds(c1_small, session, capfd):
    """GROUP BY latency: a numeric key with ~95k distinct values — eligible at
    plan build, but 16 B x groups exceeds the 64 KiB LDS table at execute."""
    q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "f_i64"}],
         "group_by": ["latency"]}
    _check(c1_small, session, q, capfd, "fallback")


def test_old_path_three_aggregates(c1, session, capfd):
    q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"},
                    {"agg": "min", "col": "latency"}],
         "group_by": ["host"]}
    _check(c1, session, q, capfd, "old")


def test_null_bearing_key_keeps_def_level_path(c5, session, capfd):
    """opt_tag is 30 % NULL: its key task keeps the def-level / scratch /
    expand launches (the null-free `host` key in the cases above takes the
    single-launch mode)."""
    q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"}],
         "group_by": ["opt_tag"]}
    rows = _check(c5, session, q, capfd, "fused")
    assert sum(r[1] for r in rows) == 100_000
