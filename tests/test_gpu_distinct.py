"""count_distinct on the GPU: the bitmap path (k_distinct_mark +
k_distinct_emit), the hash-set path (k_distinct_claim), the list-state
partial export and its Final merge. Expected values come from
tests/distinct_common.py (plain Python over the parquet files); the path each
distinct agg took is read from the GPUQ_PLAN_DEBUG line
  [gpuq exec] part <p>: distinct agg=<i> col=<c> path=bitmap|hash
      groups=<G> card=<V> pairs=<P> [mark=lds|global]
(mark: whether the bitmap path marked through a block-local LDS copy, taken
up to GPUQ_DISTINCT_LDS_BITS, or in global memory).

Data: c6, 60,000 rows in three 20,000-row one-minute files. `level` is a
dict column (12 values, 10 % NULL), `tag` runs in hash mode (PLAIN fallback
pages, 1,500 values, 30 % NULL), `opt_i64` is numeric (50 % NULL, ~30k
values), `latency` is required, `sparse` is all-NULL in the odd minute."""

import os
import re

import pyarrow as pa
import pytest

from tests import distinct_common as dc
from tests import strpred_common as sc

pytestmark = pytest.mark.gpu

BASE, MIN = sc.BASE, sc.MIN
MODES = ["bitmap", "hash"]
KNOBS = ("GPUQ_DISTINCT_FORCE_HASH", "GPUQ_DISTINCT_BITMAP_BITS",
         "GPUQ_DISTINCT_PAIR_CAP", "GPUQ_DISTINCT_LDS_BITS")
LDS_BITS = 1 << 17   # default of GPUQ_DISTINCT_LDS_BITS
MINUTE_BIN = {"bin": "p_timestamp", "stride_ms": MIN, "origin": 0}


def cd(col):
    return {"agg": "count_distinct", "col": col}


@pytest.fixture(scope="module")
def c6(tmp_path_factory):
    from datagen.gen import gen_stream

    td = tmp_path_factory.mktemp("distinct_c6")
    info = gen_stream(str(td), "s", "c6", **sc.GEN)
    info["data"] = sc.load(info["files"])
    return info


@pytest.fixture(scope="module")
def session():
    from parseable_amd import GpuSession

    return GpuSession()


def _env(mode=None, **knobs):
    env = {k: str(v) for k, v in knobs.items()}
    if mode == "hash":
        env["GPUQ_DISTINCT_FORCE_HASH"] = "1"
    return env


def _with_env(env, fn):
    """The knobs are read at plan build: set them around fn only."""
    for k in KNOBS:
        assert k not in os.environ
    os.environ["GPUQ_PLAN_DEBUG"] = "1"
    os.environ.update(env)
    try:
        return fn()
    finally:
        os.environ.pop("GPUQ_PLAN_DEBUG", None)
        for k in env:
            os.environ.pop(k, None)


def _lines(err):
    """-> [{agg, col, path, groups, card, pairs, mark}] from the exec debug
    lines (mark is None on the hash path)"""
    out = []
    for m in re.finditer(
            r"\[gpuq exec\] part \d+: distinct agg=(\d+) col=(\S+) path=(\S+) "
            r"groups=(\d+) card=(\d+) pairs=(\d+)(?: mark=(\S+))?", err):
        out.append({"agg": int(m.group(1)), "col": m.group(2),
                    "path": m.group(3), "groups": int(m.group(4)),
                    "card": int(m.group(5)), "pairs": int(m.group(6)),
                    "mark": m.group(7)})
    return out


def _gpu(info, session, q, capfd, env):
    from parseable_amd import Query, StandardTableProvider

    def run():
        capfd.readouterr()
        prov = StandardTableProvider(info["stream_dir"], session)
        rows, metrics = Query(prov).execute(dict(q))
        return rows, metrics, capfd.readouterr().err

    return _with_env(env, run)


def _check(info, session, q, capfd, mode, expect=None, **knobs):
    """Run q in `mode` (auto, named by the path it should pick: "bitmap"; or
    "hash": forced), compare with the Python reference, assert every distinct
    agg took the path `expect` (default: `mode`).
    -> (rows, expected rows, debug lines)"""
    from oracle.compare import assert_rows_equal

    rows, _, err = _gpu(info, session, q, capfd, _env(mode, **knobs))
    want = dc.expected(info["data"], q)
    assert_rows_equal(rows, want, f"GPU vs python ({mode}): {q}")
    lines = _lines(err)
    n_distinct = sum(a["agg"] == "count_distinct" for a in q["select"])
    assert len(lines) == n_distinct, err[-2000:]
    for ln in lines:
        assert q["select"][ln["agg"]] == cd(ln["col"]), ln
        assert ln["path"] == (expect or mode), (ln, err[-2000:])
        # the marking variant follows from the bitmap's size alone
        bits = ln["groups"] * ((ln["card"] + 1 + 63) // 64 * 64)
        lds_bits = int(knobs.get("GPUQ_DISTINCT_LDS_BITS", LDS_BITS))
        assert ln["mark"] == (None if ln["path"] == "hash" else
                              "lds" if bits <= lds_bits else "global"), ln
    assert "fused_count=0 fused_valagg=0" in err
    return rows, want, lines


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("col", ["level", "tag", "opt_i64", "latency",
                                 "p_timestamp", "sparse"])
def test_no_group(c6, session, capfd, col, mode):
    rows, _, lines = _check(c6, session, {"select": [cd(col)]}, capfd, mode)
    n = len({v for v in c6["data"][col] if v is not None})
    assert rows == [[n]] and n > 0
    # every claimed pair is one distinct value; the gid space covers them
    assert lines[0]["groups"] == 1 and lines[0]["pairs"] == n
    assert lines[0]["card"] >= n
    assert lines[0]["mark"] == ("lds" if mode == "bitmap" else None)


GROUPED = {
    "level->tag": {"select": [cd("tag")], "group_by": ["level"]},
    "tag->level": {"select": [cd("level")], "group_by": ["tag"]},
    "two keys": {"select": [cd("tag")], "group_by": ["level", "sparse"]},
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(GROUPED))
def test_grouped(c6, session, capfd, name, mode):
    rows, want, lines = _check(c6, session, GROUPED[name], capfd, mode)
    assert len(rows) > 10 and lines[0]["groups"] >= len(rows)
    assert lines[0]["pairs"] == sum(r[-1] for r in rows)
    assert any(r[-1] > 1 for r in rows)
    if mode == "bitmap":   # both marking variants are among the cases
        assert lines[0]["mark"] == ("global" if name == "two keys" else "lds")


@pytest.mark.parametrize("mode", MODES)
def test_date_bin_all_null_bins_are_zero(c6, session, capfd, mode):
    q = {"select": [{"agg": "count_star"}, cd("sparse")],
         "group_by": [MINUTE_BIN]}
    rows, _, _ = _check(c6, session, q, capfd, mode)
    assert [r[0] for r in rows] == [BASE, BASE + MIN, BASE + 2 * MIN]
    # the odd minute holds rows, all with a NULL sparse: 0, never NULL
    assert rows[1][1] > 0 and rows[1][2] == 0
    assert rows[0][2] == 40 and rows[2][2] == 40


def test_bitmap_threshold(c6, session, capfd):
    """G x Vpad bits: at the threshold the bitmap runs, one bit below the
    plan falls to the hash set by itself."""
    q = GROUPED["level->tag"]
    _, _, lines = _check(c6, session, q, capfd, "bitmap")
    vpad = (lines[0]["card"] + 1 + 63) // 64 * 64   # card + the null slot
    bits = lines[0]["groups"] * vpad
    assert lines[0]["groups"] == 13 and vpad == 1536
    _check(c6, session, q, capfd, "bitmap", GPUQ_DISTINCT_BITMAP_BITS=bits)
    _check(c6, session, q, capfd, "bitmap", expect="hash",
           GPUQ_DISTINCT_BITMAP_BITS=bits - 1)
    # and the LDS-copy threshold inside the bitmap path
    for lds_bits, mark in ((bits, "lds"), (bits - 1, "global"), (0, "global")):
        _, _, lines = _check(c6, session, q, capfd, "bitmap",
                             GPUQ_DISTINCT_LDS_BITS=lds_bits)
        assert lines[0]["mark"] == mark


@pytest.mark.parametrize("mode", MODES)
def test_masking(c6, session, capfd, mode):
    """A time range and a string predicate select a strict subset: a kernel
    that ignored the mask would return the all-rows answer."""
    sel = [cd("tag"), cd("level"), cd("opt_i64")]
    q = {"select": sel,
         "preds": [{"col": "message", "op": "contains", "lit": "rror"}],
         "time_range": [BASE + MIN + 5_000, BASE + MIN + 45_000]}
    rows, want, _ = _check(c6, session, q, capfd, mode)
    full = dc.expected(c6["data"], {"select": sel})
    assert 0 < want[0][0] < full[0][0] and 0 < want[0][2] < full[0][2]
    # NULL never counts: level has 12 values and a NULL
    assert None in c6["data"]["level"]
    assert 0 < rows[0][1] <= 12 and full[0][1] == 12
    # grouped too
    q = dict(q, select=[cd("tag")], group_by=["level"])
    rows, want, _ = _check(c6, session, q, capfd, mode)
    allrows = dc.expected(c6["data"], {"select": [cd("tag")],
                                       "group_by": ["level"]})
    assert sum(r[1] for r in want) < sum(r[1] for r in allrows)


OTHER_AGGS = {
    "alongside": {"select": [{"agg": "count_star"},
                             {"agg": "sum", "col": "latency"},
                             {"agg": "count", "col": "tag"}, cd("tag"),
                             {"agg": "avg", "col": "latency"}],
                  "group_by": ["level"]},
    "key is value (hash)": {"select": [cd("tag"), {"agg": "count_star"}],
                            "group_by": ["tag"]},
    "key is value (dict)": {"select": [cd("level")], "group_by": ["level"]},
    "key is value (numeric)": {"select": [cd("latency")],
                               "group_by": ["latency"]},
    "three distinct": {"select": [cd("level"), {"agg": "count_star"},
                                  cd("opt_i64"), cd("tag")],
                       "group_by": ["sparse"]},
    "same column twice": {"select": [cd("tag"), cd("tag")]},
    "min/max of the value (dict)": {
        "select": [{"agg": "min", "col": "level"}, cd("level"),
                   {"agg": "max", "col": "level"}], "group_by": ["sparse"]},
    "min/max of the value (hash)": {
        "select": [{"agg": "min", "col": "tag"}, cd("tag"),
                   {"agg": "max", "col": "tag"}], "group_by": ["level"]},
    "sum/min of the value (numeric)": {
        "select": [{"agg": "sum", "col": "opt_i64"}, cd("opt_i64"),
                   {"agg": "min", "col": "opt_i64"},
                   {"agg": "count", "col": "opt_i64"}], "group_by": ["level"]},
    "predicate on the value": {
        "select": [cd("tag"), cd("opt_i64")],
        "preds": [{"col": "tag", "op": "starts_with", "lit": "Tag-"},
                  {"col": "opt_i64", "op": "between", "lo": 0,
                   "hi": 10 ** 9}]},
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(OTHER_AGGS))
def test_with_other_aggs(c6, session, capfd, name, mode):
    q = OTHER_AGGS[name]
    # ~58k groups x ~58k values is far beyond the default 2^28 bitmap bits:
    # that plan takes the hash set without being forced
    expect = "hash" if name == "key is value (numeric)" else mode
    rows, _, _ = _check(c6, session, q, capfd, mode, expect=expect)
    if name.startswith("key is value"):
        # one value per non-NULL group, none in the NULL group
        assert all(r[1] == (0 if r[0] is None else 1) for r in rows)
        assert len(rows) > 10


@pytest.mark.parametrize("mode", MODES)
def test_cascade(c6, session, capfd, mode):
    """tag x opt_i64: the dense key product exceeds 2^22, the keys combine
    through the pair cascade and the distinct pass reads the combined gid."""
    q = {"select": [{"agg": "count_star"}, cd("level")],
         "group_by": ["tag", "opt_i64"]}
    data = c6["data"]
    n_tag = len({v for v in data["tag"] if v is not None})
    n_opt = len({v for v in data["opt_i64"] if v is not None})
    assert (n_tag + 1) * (n_opt + 1) > 1 << 22
    rows, _, lines = _check(c6, session, q, capfd, mode)
    assert lines[0]["groups"] == len(rows) > 10_000
    assert lines[0]["mark"] == ("global" if mode == "bitmap" else None)
    assert {r[3] for r in rows} >= {0, 1} and max(r[3] for r in rows) > 2


def _subset(data, files):
    keep = [i for i, f in enumerate(data["__file"]) if f in files]
    return {c: [v[i] for i in keep] for c, v in data.items()}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("q", [
    {"select": [{"agg": "count_star"}, cd("tag")], "group_by": ["level"]},
    {"select": [cd("latency"), cd("level")]},
], ids=["grouped-hash-utf8", "nogroup-numeric-dict"])
def test_partials_union(c6, session, capfd, q, mode):
    """Two plans over disjoint file subsets: the Final merge unions the
    agg{i}_set lists — the reference over all rows, less than the sum of the
    two local counts."""
    from oracle.compare import assert_rows_equal
    from parseable_amd.provider import (GpuExecutionPlan, distinct_set_columns,
                                        merge_partials)

    data, files = c6["data"], c6["files"]
    nk = len(q.get("group_by", []))
    set_cols = distinct_set_columns(q["select"], nk)
    fixed = nk + 1 + 2 * len(q["select"])

    def partial(paths):
        plan = GpuExecutionPlan(session, paths, dict(q))
        try:
            assert plan.partition_count() == 1
            return plan.execute(0)
        finally:
            plan.close()

    b0, b1 = _with_env(_env(mode), lambda: (partial(files[:2]),
                                            partial(files[2:])))
    err = capfd.readouterr().err
    assert [ln["path"] for ln in _lines(err)] == [mode] * (2 * len(set_cols))
    for b, fs in ((b0, {0, 1}), (b1, {2})):
        sub = _subset(data, fs)
        assert b.num_columns == fixed + len(set_cols)
        assert_rows_equal(merge_partials([b], q), dc.expected(sub, q),
                          "one partial is final")
        keys = list(zip(*[b.column(k).to_pylist() for k in range(nk)])) \
            if nk else [()] * b.num_rows
        for i, ci in set_cols.items():
            field, col = b.schema.field(ci), b.column(ci)
            assert field.name == f"agg{i}_set"
            want_t = {"tag": pa.string(), "level": pa.string(),
                      "latency": pa.int64()}[q["select"][i]["col"]]
            assert col.type == pa.list_(want_t) and col.null_count == 0
            want_sets = dc.group_sets(sub, q, i)
            got = col.to_pylist()
            assert len(got) == len(want_sets)
            for key, vals in zip(keys, got):
                key = tuple(k.encode() if isinstance(k, str) else k
                            for k in key)
                enc = [v.encode() if isinstance(v, str) else v for v in vals]
                assert len(enc) == len(set(enc))          # no duplicates
                assert set(enc) == want_sets[key], key
            lens = [len(v) for v in got]
            assert lens == b.column(nk + 1 + 2 * i).to_pylist()
            assert lens == b.column(nk + 2 + 2 * i).to_pylist()
    merged = merge_partials([b0, b1], q)
    assert_rows_equal(merged, dc.expected(data, q), "union of two partials")
    for i in set_cols:
        total = sum(r[nk + i] for r in merged)
        local = sum(sum(r[nk + i] for r in merge_partials([b], q))
                    for b in (b0, b1))
        assert total < local, (i, total, local)


@pytest.mark.parametrize("mode", MODES)
def test_pair_cap_raises_and_session_survives(c6, session, capfd, mode):
    """More distinct pairs than the (lowered) cap: the kernels report the cap
    through the error word — no fault — and the session keeps working."""
    from parseable_amd.provider import GpuqError

    q = {"select": [cd("opt_i64")]}
    with pytest.raises(GpuqError) as ei:
        _gpu(c6, session, q, capfd, _env(mode, GPUQ_DISTINCT_PAIR_CAP=1000))
    msg = str(ei.value)
    assert "more than 1000 distinct (group, value) pairs" in msg, msg
    assert "GPUQ_DISTINCT_PAIR_CAP" in msg
    _check(c6, session, q, capfd, mode)
    # at the cap exactly it still fits
    n = len({v for v in c6["data"]["opt_i64"] if v is not None})
    _check(c6, session, q, capfd, mode, GPUQ_DISTINCT_PAIR_CAP=n)
    with pytest.raises(GpuqError):
        _gpu(c6, session, q, capfd, _env(mode, GPUQ_DISTINCT_PAIR_CAP=n - 1))


@pytest.mark.parametrize("mode", MODES)
def test_same_query_twice(c6, session, capfd, mode):
    q = {"select": [{"agg": "count_star"}, cd("tag"), cd("opt_i64")],
         "group_by": ["level"]}
    rows1, m1, _ = _gpu(c6, session, q, capfd, _env(mode))
    rows2, m2, _ = _gpu(c6, session, q, capfd, _env(mode))
    assert rows1 == rows2 == dc.expected(c6["data"], q)
    # the second run is served by the hot tier
    assert m2["cache_hit_bytes"] == m2["bytes_scanned"] > 0
