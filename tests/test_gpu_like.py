"""General LIKE / ILIKE patterns (like / not_like / ilike / not_ilike) on the
GPU: k_like_win<> over PLAIN pages (its oversized-value branch included), the
per-dict-entry LUT, the STR_PATTERN branch of k_cmp_str on hash-mode columns,
canonicalised shapes and WHERE trees. Expected rows come from
tests/like_common.py (plain Python over the parquet files), the fixed counts
from its tables; the path each predicate took is read from the
GPUQ_PLAN_DEBUG lines
  [gpuq plan] pred <i> col=<c> op=<op> path=lut|lut+window|hash[ as=<op>]

Data: c6, 60,000 rows in three 20,000-row files (strpred_common.GEN)."""

import os
import re

import pytest

from tests import like_common as lc
from tests import strpred_common as sc

pytestmark = pytest.mark.gpu

BASE, MIN = sc.BASE, sc.MIN
COUNT = [{"agg": "count_star"}]


@pytest.fixture(scope="module")
def c6(tmp_path_factory):
    from datagen.gen import gen_stream

    td = tmp_path_factory.mktemp("like_c6")
    info = gen_stream(str(td), "s", "c6", **sc.GEN)
    info["data"] = sc.load(info["files"])
    for col, n in lc.NON_NULL.items():
        assert sum(v is not None for v in info["data"][col]) == n
    return info


@pytest.fixture(scope="module")
def session():
    from parseable_amd import GpuSession

    return GpuSession()


def _gpu(info, session, q, capfd):
    """-> (rows, [(col, op, path, as or None)], plan debug text)"""
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
        r"\[gpuq plan\] pred \d+ col=(\S+) op=(\S+) path=(\S+)(?: as=(\S+))?\n",
        err)
    return rows, [(c, o, p, a or None) for c, o, p, a in paths], err


def _pred(col, op, lit):
    return {"col": col, "op": op, "lit": lit}


def _check(info, session, q, capfd, n_sel=None, vacuous=False):
    """Run q and compare with the reference rows. n_sel: the count the issue
    states for this case. Unless declared vacuous, 0 < selected < non-null
    rows of the first predicate's column."""
    from oracle.compare import assert_rows_equal

    data = info["data"]
    rows, paths, err = _gpu(info, session, q, capfd)
    assert_rows_equal(rows, lc.expected(data, q), f"GPU vs python: {q}")
    got = len(lc.selected(data, q))
    if n_sel is not None:
        assert got == n_sel, (q, got, n_sel)
    if not vacuous:
        col = q["preds"][0]["col"]
        assert 0 < got < lc.NON_NULL[col], (q, got)
    return rows, paths, err


def _ops_counts(col, n_like, n_ilike):
    nn = lc.NON_NULL[col]
    out = [("like", n_like), ("not_like", nn - n_like)]
    if n_ilike is not None:
        out += [("ilike", n_ilike), ("not_ilike", nn - n_ilike)]
    return out


# 1. message: dict pages via the LUT, PLAIN pages via k_like_win
@pytest.mark.parametrize("pat,n_like,n_ilike", lc.MESSAGE_PATTERNS)
def test_message_window_and_lut(c6, session, capfd, pat, n_like, n_ilike):
    cases = _ops_counts("message", n_like, n_ilike)
    if n_ilike is None and pat.isascii():
        cases += [("ilike", None), ("not_ilike", None)]
    for op, n in cases:
        q = {"select": COUNT, "preds": [_pred("message", op, pat)]}
        rows, paths, err = _check(c6, session, q, capfd, n_sel=n)
        assert paths == [("message", op, "lut+window", None)], paths
        if n is not None:
            assert rows == [[n]]
        m = re.search(r"\[gpuq plan\] part 0: .* cwins=(\d+)", err)
        assert m and int(m.group(1)) > 0, err[-1500:]


@pytest.mark.parametrize("pat,n_like", lc.MESSAGE_VACUOUS)
def test_message_all_or_none(c6, session, capfd, pat, n_like):
    nn = lc.NON_NULL["message"]
    for op, n in (("like", n_like), ("not_like", nn - n_like),
                  ("ilike", n_like), ("not_ilike", nn - n_like)):
        q = {"select": COUNT, "preds": [_pred("message", op, pat)]}
        rows, paths, _ = _check(c6, session, q, capfd, n_sel=n, vacuous=True)
        assert rows == [[n]], (op, pat, rows)
        assert paths[0][2] == "lut+window"
        # '%' alone is the empty-literal CONTAINS and '%\\%%' is '%lit%' with
        # the literal '%'; the third has an inner '%' and stays general
        neg = "not_" if op.startswith("not_") else ""
        fold = "i" if op.endswith("ilike") else ""
        assert paths[0][3] == {"%": neg + "contains",
                               "%\\%%": neg + fold + "contains"}.get(pat)


# 2. '_' is one character, not one byte
@pytest.mark.parametrize("pat,n_like", lc.MULTIBYTE_PATTERNS)
def test_multibyte_underscore(c6, session, capfd, pat, n_like):
    for op, n in _ops_counts("message", n_like, None):
        q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"}],
             "group_by": ["level"], "preds": [_pred("message", op, pat)]}
        _, paths, _ = _check(c6, session, q, capfd, n_sel=n)
        assert paths == [("message", op, "lut+window", None)], paths


# 3. the run of '='-filled messages in minute 1
@pytest.mark.parametrize("pat,n_like,n_ilike", lc.DENSE_PATTERNS)
def test_dense_run(c6, session, capfd, pat, n_like, n_ilike):
    cases = [("like", n_like)] + ([("ilike", n_ilike)] if n_ilike else [])
    for op, n in cases:
        q = {"select": COUNT, "preds": [_pred("message", op, pat)]}
        rows, paths, _ = _check(c6, session, q, capfd, n_sel=n)
        assert rows == [[n]]
        assert paths == [("message", op, "lut+window", None)], paths
        q["time_range"] = [BASE + MIN, BASE + 2 * MIN]
        _check(c6, session, q, capfd, n_sel=n)


# 4. the 40,000-byte message: the single-value branch of k_like_win
@pytest.mark.parametrize("pat", lc.BIG_PATTERNS)
def test_oversized_value(c6, session, capfd, pat):
    data = c6["data"]
    big = [i for i, v in enumerate(data["message"])
           if v is not None and len(v) > 16384]
    assert len(big) == 1 and len(data["message"][big[0]]) == 40_000
    q = {"select": COUNT, "preds": [_pred("message", "like", pat)]}
    assert lc.selected(data, q) == big
    rows, paths, _ = _check(c6, session, q, capfd, n_sel=1)
    assert rows == [[1]]
    assert paths == [("message", "like", "lut+window", None)], paths
    q = {"select": COUNT, "preds": [_pred("message", "not_like", pat)]}
    rows, _, _ = _check(c6, session, q, capfd, n_sel=45_489)
    assert rows == [[45_489]]
    # folded, and narrowed to the value's minute
    q = {"select": COUNT, "preds": [_pred("message", "ilike", pat.swapcase())],
         "time_range": [BASE, BASE + MIN]}
    assert big[0] in lc.selected(data, q)
    _check(c6, session, q, capfd)
    # projection: the row's timestamp comes back
    q = {"select_cols": ["p_timestamp", "level", "latency"], "limit": 5,
         "preds": [_pred("message", "like", pat)]}
    rows, _, _ = _gpu(c6, session, q, capfd)
    want = [[data[c][big[0]] for c in q["select_cols"]]]
    want[0][1] = want[0][1].decode() if want[0][1] is not None else None
    assert rows == want, (rows, want)


# 5. level: dictionary pages only
@pytest.mark.parametrize("pat,n_like,n_ilike", lc.LEVEL_PATTERNS)
def test_level_lut(c6, session, capfd, pat, n_like, n_ilike):
    for op, n in _ops_counts("level", n_like, n_ilike):
        q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"}],
             "group_by": ["level"], "preds": [_pred("level", op, pat)]}
        _, paths, _ = _check(c6, session, q, capfd, n_sel=n)
        assert paths == [("level", op, "lut", None)], paths


# 6. tag: a group key with PLAIN pages -> hash mode, k_cmp_str
@pytest.mark.parametrize("pat,n_like,n_ilike", lc.TAG_PATTERNS)
def test_tag_hash_mode(c6, session, capfd, pat, n_like, n_ilike):
    for op, n in _ops_counts("tag", n_like, n_ilike):
        q = {"select": COUNT, "group_by": ["tag"],
             "preds": [_pred("tag", op, pat)]}
        _, paths, _ = _check(c6, session, q, capfd, n_sel=n)
        assert paths == [("tag", op, "hash", None)], paths


# 7. canonicalised shapes run as the existing op
@pytest.mark.parametrize("op,pat,as_op,lit", [
    ("like", "%rror%", "contains", "rror"),
    ("like", "Error%", "starts_with", "Error"),
    ("like", "%TIMEOUT", "ends_with", "TIMEOUT"),
    ("ilike", "%error%", "icontains", "error"),
    ("not_like", "%rror%", "not_contains", "rror"),
    ("not_ilike", "%ERROR%", "not_icontains", "error"),
])
def test_canonical_shapes(c6, session, capfd, op, pat, as_op, lit):
    sel = [{"agg": "count_star"}, {"agg": "max", "col": "latency"}]
    q = {"select": sel, "group_by": ["level"],
         "preds": [_pred("message", op, pat)]}
    rows, paths, _ = _check(c6, session, q, capfd)
    assert paths == [("message", op, "lut+window", as_op)], paths
    q0 = {"select": sel, "group_by": ["level"],
          "preds": [_pred("message", as_op, lit)]}
    rows0, paths0, _ = _gpu(c6, session, q0, capfd)
    assert paths0 == [("message", as_op, "lut+window", None)], paths0
    assert rows == rows0


# 8. combinations
def test_conjunctions(c6, session, capfd):
    q = {"select": COUNT,
         "preds": [_pred("message", "like", "%_rror%"),
                   _pred("message", "not_contains", "TIMEOUT"),
                   _pred("message", "not_ilike", "%zone%queue%")]}
    _, paths, _ = _check(c6, session, q, capfd)
    assert [p[2] for p in paths] == ["lut+window"] * 3
    q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"}],
         "group_by": ["level"],
         "preds": [_pred("message", "ilike", "err_r%"),
                   _pred("level", "not_like", "E%R")],
         "time_range": [BASE + MIN + 5_000, BASE + 2 * MIN + 45_000]}
    _, paths, _ = _check(c6, session, q, capfd)
    assert [p[2] for p in paths] == ["lut+window", "lut"]
    q = {"select": COUNT, "group_by": ["tag"],
         "preds": [_pred("tag", "like", "T%-0001__"),
                   _pred("tag", "not_ends_with", "7")]}
    _, paths, _ = _check(c6, session, q, capfd)
    assert [p[2] for p in paths] == ["hash", "hash"]


def test_where_trees(c6, session, capfd):
    from oracle.compare import assert_rows_equal

    data = c6["data"]
    sel = [{"agg": "count_star"}, {"agg": "max", "col": "latency"}]
    # two columns: each leaf into the OR group's scratch mask
    q = {"select": sel, "group_by": ["level"],
         "where": {"or": [_pred("message", "like", "Err_r%"),
                          _pred("level", "ilike", "w__n")]}}
    rows, paths, err = _gpu(c6, session, q, capfd)
    assert_rows_equal(rows, lc.expected(data, q), str(q))
    n = len(lc.selected(data, q))
    n_a = lc.count(data, "message", "like", "Err_r%")
    n_b = lc.count(data, "level", "ilike", "w__n")
    assert max(n_a, n_b) < n < n_a + n_b   # a real union, with an overlap
    assert re.search(r"\[gpuq plan\] or node=\d+ terms=2 path=mask", err), err
    # one dictionary column: the group folds into a single LUT
    q = {"select": sel, "group_by": ["level"],
         "where": {"or": [_pred("level", "like", "E%R"),
                          _pred("level", "like", "W__N")]}}
    rows, paths, err = _gpu(c6, session, q, capfd)
    assert_rows_equal(rows, lc.expected(data, q), str(q))
    assert len(lc.selected(data, q)) == 4432 + 4537
    assert re.search(r"\[gpuq plan\] or node=\d+ terms=2 path=lut", err), err
    assert [p[2] for p in paths] == ["lut", "lut"]
    # an OR next to a conjunct, a nested AND, new ops mixed with an old one
    q = {"select": COUNT,
         "preds": [_pred("message", "not_like", "")],
         "where": {"or": [_pred("message", "like", "%caf_ %"),
                          {"and": [_pred("tag", "like", "Tag-%7"),
                                   _pred("message", "icontains", "error")]}]}}
    rows, _, _ = _gpu(c6, session, q, capfd)
    assert_rows_equal(rows, lc.expected(data, q), str(q))
    n = len(lc.selected(data, q))
    assert 18_793 < n < lc.NON_NULL["message"]


# 9. the seeded random patterns of the CPU test (which asserts, from the
# reference alone, that at least half of them split the column), five a case
@pytest.mark.parametrize("k", range(lc.N_RANDOM // 5))
def test_random_patterns(c6, session, capfd, k):
    pats = lc.random_patterns()[5 * k:5 * k + 5]
    assert len(pats) == 5
    for pat in pats:
        q = {"select": COUNT, "preds": [_pred("message", "like", pat)]}
        _check(c6, session, q, capfd, vacuous=True)
        if pat.isascii():
            q = {"select": COUNT, "preds": [_pred("message", "not_ilike", pat)]}
            _check(c6, session, q, capfd, vacuous=True)
