"""Expected values for the per-aggregate FILTER tests
(`{"agg": ..., "filter": <leaf | {"and": [...]} | {"or": [...]}>}` in
query["select"]), in plain Python over `where_common.load` data. The oracle
does not know filters; this reference is `where_common.expected` with, per
aggregate, the row set `selected(data, query) & node_rows(data, filter)`.

Semantics (include/gpuq.h): groups are decided by WHERE alone — a group whose
rows all fail a filter stays, with 0 for count_star / count / count_distinct
and None for sum / min / max / avg; with no group-by there is always one row.

f64 sums are the correctly rounded exact sum (math.fsum), which the engine's
superaccumulator produces too; `cross_check` ties every column to
`where_common.expected` on the unfiltered query with WHERE AND filter, whose
f64 sums add in row order — floats compare there within oracle.compare's
FLOAT_RTOL, everything else exactly."""

import math

from tests import where_common as wc

COUNT_AGGS = ("count_star", "count", "count_distinct")


def strip(query):
    """The query without its filters."""
    return dict(query, select=[{k: v for k, v in a.items() if k != "filter"}
                               for a in query["select"]])


def has_filter(query):
    return any(a.get("filter") is not None for a in query["select"])


_ROWS = {}


def node_rows(data, node):
    """where_common.node_rows with the leaf row sets kept per data set — the
    GPU tests reuse a few dozen leaves over hundreds of queries."""
    k = wc.group_kind(node)
    if k is None:
        key = (id(data), repr(node))
        if key not in _ROWS:
            _ROWS[key] = frozenset(wc.node_rows(data, node))
        return _ROWS[key]
    sets = [node_rows(data, kid) for kid in node[k]]
    out = sets[0]
    for s in sets[1:]:
        out = out & s if k == "and" else out | s
    return out


def selected(data, query):
    """where_common.selected over the kept leaf row sets."""
    rows = None
    for kid in wc.root_node(query):
        r = node_rows(data, kid)
        rows = r if rows is None else rows & r
    if rows is None:
        return list(range(len(data["p_timestamp"])))
    return sorted(rows)


def _final(a, vals):
    """One aggregate over the non-NULL-filtered value list of a group (for
    count_star: one entry per row)."""
    kind = a["agg"]
    if kind in ("count_star", "count"):
        return len(vals)
    if kind == "count_distinct":
        return len(set(vals))
    if not vals:
        return None
    if kind in ("sum", "avg"):
        s = math.fsum(vals) if isinstance(vals[0], float) else sum(vals)
        return s / len(vals) if kind == "avg" else s
    return min(vals) if kind == "min" else max(vals)


def expected(data, query):
    """Rows in the engine's normalized form: [key..., agg...] sorted by key,
    NULL keys last."""
    idx = selected(data, query)
    gb = query.get("group_by", [])
    aggs = query["select"]
    fsets = [None if a.get("filter") is None
             else node_rows(data, a["filter"]) for a in aggs]
    acc = {}
    for i in idx:
        key = tuple(data[g][i] for g in gb)
        st = acc.setdefault(key, [[] for _ in aggs])
        for k, a in enumerate(aggs):
            if fsets[k] is not None and i not in fsets[k]:
                continue
            if a["agg"] == "count_star":
                st[k].append(1)
                continue
            v = data[a["col"]][i]
            if v is not None:
                st[k].append(v)
    if not gb and not acc:
        acc[()] = [[] for _ in aggs]
    rows = []
    for key in sorted(acc, key=lambda k: tuple(
            (1, b"") if v is None else (0, v) for v in k)):
        rows.append([wc._out(v) for v in key]
                    + [wc._out(_final(a, acc[key][k]))
                       for k, a in enumerate(aggs)])
    return rows


def cross_check(data, query):
    """For every aggregate i: column i of expected() equals
    where_common.expected on the unfiltered query with WHERE AND filter_i,
    left-joined onto the groups of the WHERE-only query with 0 / None."""
    from oracle.compare import FLOAT_RTOL, values_equal

    nk = len(query.get("group_by", []))
    mine = expected(data, query)
    plain = strip(query)
    groups = [tuple(r[:nk]) for r in wc.expected(data, plain)]
    assert [tuple(r[:nk]) for r in mine] == groups, query
    for i, a in enumerate(plain["select"]):
        q = dict(plain, select=[a])
        f = query["select"][i].get("filter")
        if f is not None:
            q["preds"] = list(plain.get("preds", [])) + [f]
        got = {tuple(r[:nk]): r[nk] for r in wc.expected(data, q)}
        fill = 0 if a["agg"] in COUNT_AGGS else None
        for r in mine:
            want = wc._out(got.get(tuple(r[:nk]), fill))
            assert values_equal(r[nk + i], want, float_rtol=FLOAT_RTOL), (
                query, i, r, want)
