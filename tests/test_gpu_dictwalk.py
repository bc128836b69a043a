"""dict_page_decode's run-header scan against the fixtures of
tests/dictwalk_common.py (tests/test_dictwalk_cpu.py proves that each file
holds the run structure it is named for), through every consumer of the
decoder and under both walks: the default 64-way scan and
GPUQ_DICT_WALK=serial, the one-header-per-step walk.

All fixtures of a variant are ONE plan (a file is a row group): the group
key k is distinct per file, so a result row of a query grouped by k belongs
to one fixture, and one query per consumer covers every shape. Expected
rows come from pc.ref_query over the source arrays (plain Python, exact
ints), computed once per query and shared by both walks; the two walks must
also agree with each other row for row.

Consumers and the queries that reach them (null-free files, mode 2):
  EmitGidP, EmitDictMaskP, EmitDictI64P   group by s, s != lit, min(x)
  EmitValAgg<K1, MASK>                    count + sum|min|max(x) by k, s != lit
  EmitValAgg<K1, no mask>                 count + sum|min|max(x) by k
  EmitDictI64P                            both under GPUQ_NO_FUSED_VALAGG=1
_nul files (modes 0 and 1 with present[], k_expand):
  EmitGidP, EmitDictMaskP, EmitLutD       group by s, s != lit
  EmitDictI64P                            min/sum(x) by k
  EmitDictMaskP, EmitLutD                 count where s = lit
The 20-bit file runs alone (524,289 dictionary entries): fused and
materialised max(x) by k.

The page split of the first design (several blocks per page) did not pay
and was removed with its GPUQ_DICT_SPLIT switch, so
the settings are the two walks.
"""

import os
import re

import pytest

from tests import dictwalk_common as dw
from tests import pagecases_common as pc

pytestmark = pytest.mark.gpu

WALKS = {"scan": {}, "serial": {"GPUQ_DICT_WALK": "serial"}}
LIT = "v0000003"

NE = [{"col": "s", "op": "ne", "lit": LIT}]
QUERIES = {
    # name: (fixture set, query, extra env, expected plan path or None)
    "gid_mask_i64": ("nn", {"select": [{"agg": "count_star"},
                                       {"agg": "max", "col": "o"},
                                       {"agg": "min", "col": "x"}],
                            "group_by": ["s"], "preds": NE}, {}, "old"),
    "valagg_masked": ("nn", {"select": [{"agg": "count_star"},
                                        {"agg": "max", "col": "x"}],
                             "group_by": ["k"], "preds": NE}, {}, "fused"),
    "valagg_sum": ("nn", {"select": [{"agg": "count_star"},
                                     {"agg": "sum", "col": "x"}],
                          "group_by": ["k"]}, {}, "fused"),
    "valagg_min_masked": ("nn", {"select": [{"agg": "count_star"},
                                            {"agg": "min", "col": "x"}],
                                 "group_by": ["k"], "preds": NE}, {}, "fused"),
    "valagg_min": ("nn", {"select": [{"agg": "count_star"},
                                     {"agg": "min", "col": "x"}],
                          "group_by": ["k"]}, {}, "fused"),
    "valagg_max": ("nn", {"select": [{"agg": "count_star"},
                                     {"agg": "max", "col": "x"}],
                          "group_by": ["k"]}, {}, "fused"),
    "valagg_sum_masked": ("nn", {"select": [{"agg": "count_star"},
                                            {"agg": "sum", "col": "x"}],
                                 "group_by": ["k"], "preds": NE}, {}, "fused"),
    "nul_gid_mask": ("nul", {"select": [{"agg": "count_star"},
                                        {"agg": "count", "col": "x"},
                                        {"agg": "max", "col": "o"}],
                             "group_by": ["s"], "preds": NE}, {}, "old"),
    "nul_i64": ("nul", {"select": [{"agg": "count_star"},
                                   {"agg": "min", "col": "x"},
                                   {"agg": "sum", "col": "x"}],
                        "group_by": ["k"]}, {}, "old"),
    "nul_eq": ("nul", {"select": [{"agg": "count_star"}],
                       "preds": [{"col": "s", "op": "eq", "lit": LIT}]},
               {}, None),
    "big_valagg": ("big", {"select": [{"agg": "count_star"},
                                      {"agg": "max", "col": "x"}],
                           "group_by": ["k"]}, {}, "fused"),
}
NO_FUSED = {"GPUQ_NO_FUSED_VALAGG": "1"}
for _q in ("valagg_masked", "valagg_sum", "big_valagg"):
    _s, _query, _, _ = QUERIES[_q]
    QUERIES[_q + "_unfused"] = (_s, _query, NO_FUSED, "old")


@pytest.fixture(scope="module")
def fs(tmp_path_factory):
    return dw.FixtureSet(tmp_path_factory.mktemp("dictwalk_gpu"))


@pytest.fixture(scope="module")
def session():
    from parseable_amd import GpuSession

    return GpuSession()


def _cases(fs, which):
    return {"nn": lambda: fs.cases(False), "nul": lambda: fs.cases(True),
            "big": fs.big}[which]()


_ref, _got = {}, {}


def _reference(fs, which, q):
    """pc.ref_query over the merged source arrays, once per query."""
    key = (which, repr(q))
    if key not in _ref:
        _ref[key] = pc.ref_query(dw.merged(_cases(fs, which)), q)
    return _ref[key]


def _run(session, paths, q, env, capfd):
    from parseable_amd.provider import GpuExecutionPlan

    env = dict(env, GPUQ_PLAN_DEBUG="1")
    capfd.readouterr()
    os.environ.update(env)
    try:
        plan = GpuExecutionPlan(session, paths, dict(q))
        try:
            assert not plan.empty
            plan.load()
            rows = plan.execute_all()
        finally:
            plan.close()
    finally:
        for k in env:
            os.environ.pop(k, None)
    return rows, capfd.readouterr().err


def _plan_path(err):
    m = re.search(r"\[gpuq plan\] fused_count=\d fused_valagg=(\d)", err)
    assert m, "no plan debug line on fd 2:\n" + err[-2000:]
    execs = set(re.findall(r"\[gpuq exec\] part \d+: valagg=(\w+)", err))
    return "old" if m.group(1) == "0" else "+".join(sorted(execs))


def _assert_rows(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} rows, want {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        bad = pc.first_mismatch(g, w)
        assert bad is None, f"{what}: result row {i} ({g!r} vs {w!r}): {bad}"


@pytest.mark.parametrize("walk", list(WALKS))
@pytest.mark.parametrize("name", list(QUERIES))
def test_consumers(fs, session, capfd, name, walk):
    which, q, env, path = QUERIES[name]
    cases = _cases(fs, which)
    rows, err = _run(session, [c.path for c in cases], q,
                     dict(env, **WALKS[walk]), capfd)
    if path is not None:
        assert _plan_path(err) == path, err[-2000:]
    # the debug line echoes the plan's setting; that the scan really accepts
    # runs is not visible from outside. It is covered by comparing the two
    # walks on pages whose run structure tests/test_dictwalk_cpu.py proves:
    # a scan that accepted nothing would equal the serial walk trivially, one
    # that accepted a wrong position would decode other rows.
    walks = set(re.findall(r"dict_walk=(\w+)", err))
    assert walks == {walk}, err[-2000:]
    _assert_rows(rows, _reference(fs, which, q), f"{name} [{walk}] vs source")
    _got[(name, walk)] = rows
    other = _got.get((name, "serial" if walk == "scan" else "scan"))
    if other is not None:
        _assert_rows(rows, other, f"{name}: {walk} vs the other walk")


def test_every_fixture_in_result(fs):
    """The reference of the k-grouped queries has rows of every file: no
    fixture drops out of the merged plan unnoticed."""
    which, q, _, _ = QUERIES["valagg_sum"]
    keys = {r[0][:4] for r in _reference(fs, which, q)}
    assert len(keys) == len(fs.shapes)
