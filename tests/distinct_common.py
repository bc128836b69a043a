"""Expected values for the count_distinct tests, in plain Python over the
parquet files (the oracle does not know the op). Built on the unmodified
tests/strpred_common.py: `load` reads the data, `selected` applies the
predicates and the time range.

Semantics (include/gpuq.h): per group, the number of distinct non-NULL values
of the column among the selected rows; a group with none gives 0, never NULL.
Group keys may be columns or DATE_BIN pseudo-keys
({"bin": col, "stride_ms": s, "origin": o})."""

from tests import strpred_common as sc

COUNT_AGGS = ("count_star", "count", "count_distinct")


def _key(data, g, i):
    if isinstance(g, dict):
        stride, origin = g["stride_ms"], g.get("origin", 0)
        ts = data[g["bin"]][i]
        return None if ts is None else origin + (ts - origin) // stride * stride
    return data[g][i]


def group_sets(data, query, agg_index):
    """{key tuple: set of the distinct agg's non-None values} over the
    selected rows; every group with a selected row has an entry."""
    col = data[query["select"][agg_index]["col"]]
    gb = query.get("group_by", [])
    out = {}
    for i in sc.selected(data, query):
        s = out.setdefault(tuple(_key(data, g, i) for g in gb), set())
        if col[i] is not None:
            s.add(col[i])
    return out


def expected(data, query):
    """Rows in the engine's normalized form: [key..., agg...] sorted by key
    with NULL keys last."""
    gb = query.get("group_by", [])
    aggs = query["select"]
    acc = {}
    for i in sc.selected(data, query):
        key = tuple(_key(data, g, i) for g in gb)
        st = acc.setdefault(key, [0, [None] * len(aggs), [0] * len(aggs)])
        st[0] += 1
        for k, a in enumerate(aggs):
            if a["agg"] == "count_star":
                continue
            v = data[a["col"]][i]
            if v is None:
                continue
            st[2][k] += 1
            cur = st[1][k]
            if a["agg"] == "count":
                continue
            if a["agg"] == "count_distinct":
                if cur is None:
                    cur = st[1][k] = set()
                cur.add(v)
            elif cur is None:
                st[1][k] = v
            elif a["agg"] in ("sum", "avg"):
                st[1][k] = cur + v
            elif a["agg"] == "min":
                st[1][k] = min(cur, v)
            elif a["agg"] == "max":
                st[1][k] = max(cur, v)
    if not gb and not acc:
        return [[0 if a["agg"] in COUNT_AGGS else None for a in aggs]]
    rows = []
    for key in sorted(acc, key=lambda k: tuple(
            (1, b"") if v is None else (0, v) for v in k)):
        st = acc[key]
        row = [sc._out(v) for v in key]
        for k, a in enumerate(aggs):
            if a["agg"] == "count_star":
                row.append(st[0])
            elif a["agg"] == "count":
                row.append(st[2][k])
            elif a["agg"] == "count_distinct":
                row.append(len(st[1][k] or ()))
            elif a["agg"] == "avg":
                row.append(st[1][k] / st[2][k] if st[2][k] else None)
            else:
                row.append(sc._out(st[1][k]))   # utf8 min / max
        rows.append(row)
    return rows
