"""Expected values for the LIKE-family / IS [NOT] NULL predicate tests,
computed in plain Python over the parquet files read with pyarrow — the
oracle does not know these ops, so the tests carry their own reference.

Semantics (include/gpuq.h): the literal is a plain byte string; the i-ops
fold ASCII A-Z only, which is exactly bytes.lower(); a NULL row satisfies no
string op, the negated ones included; only is_null selects NULL rows; an
empty literal matches every non-null row (no row when negated)."""

BASE = 1756684800000   # datagen.gen.BASE_TS_MS
MIN = 60_000
GEN = dict(rows=60_000, rows_per_file=20_000, data_page_size=65536)

STR_OPS = ["contains", "icontains", "starts_with", "ends_with", "not_contains",
           "not_icontains", "not_starts_with", "not_ends_with"]
NEW_STR_OPS = STR_OPS[1:]
NULL_OPS = ["is_null", "is_not_null"]
ABSENT = "ZZZabsentQQ"


def level_needles(op):
    """Needles that split c6's twelve `level` values for this op."""
    base = op[4:] if op.startswith("not_") else op
    return {"contains": ["E", "rror", "o"], "icontains": ["e", "RROR", "O"],
            "starts_with": ["E", "WARN", "de"],
            "ends_with": ["o", "rror", "N"]}[base]


def load(files):
    """-> {column: python list over all files (utf8 as bytes, ts as int ms)}
    plus "__file": the file index of each row."""
    import pyarrow as pa
    import pyarrow.parquet as pq

    out = {}
    for fi, f in enumerate(files):
        t = pq.read_table(f)
        for name in t.column_names:
            c = t.column(name)
            if pa.types.is_string(c.type):
                c = c.cast(pa.binary())
            elif pa.types.is_timestamp(c.type):
                c = c.cast(pa.int64())
            out.setdefault(name, []).extend(c.to_pylist())
        out.setdefault("__file", []).extend([fi] * t.num_rows)
    return out


def match(p, v):
    op = p["op"]
    if op == "is_null":
        return v is None
    if op == "is_not_null":
        return v is not None
    if v is None:
        return False
    if op == "between":
        return p["lo"] <= v and (v < p["hi"] if p.get("hi_exclusive")
                                 else v <= p["hi"])
    neg = op.startswith("not_")
    base = op[4:] if neg else op
    needle = p["lit"].encode()
    if base == "icontains":
        v, needle = v.lower(), needle.lower()
    if base == "starts_with":
        ok = v.startswith(needle)
    elif base == "ends_with":
        ok = v.endswith(needle)
    elif base in ("contains", "icontains"):
        ok = needle in v
    else:
        raise ValueError(op)
    return ok != neg


def selected(data, query):
    """Row indices satisfying every predicate and the time range."""
    preds = list(query.get("preds", []))
    tr = query.get("time_range")
    if tr:
        preds.append({"col": "p_timestamp", "op": "between", "lo": tr[0],
                      "hi": tr[1], "hi_exclusive": True})
    idx = range(len(data["p_timestamp"]))
    for p in preds:
        col = data[p["col"]]
        idx = [i for i in idx if match(p, col[i])]
    return list(idx)


def _out(v):
    return v.decode() if isinstance(v, bytes) else v


def expected(data, query):
    """Rows in the engine's normalized form: [key..., agg...] sorted by key
    with NULL keys last; or projected rows by p_timestamp DESC."""
    idx = selected(data, query)
    if query.get("select_cols"):
        cols = query["select_cols"]
        rows = [[_out(data[c][i]) for c in cols] for i in idx]
        rows.sort(key=lambda r: -r[cols.index("p_timestamp")])
        lim = query.get("limit")
        return rows[:lim] if lim else rows
    gb = query.get("group_by", [])
    aggs = query["select"]
    acc = {}
    for i in idx:
        key = tuple(data[g][i] for g in gb)
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
            if cur is None:
                st[1][k] = v
            elif a["agg"] == "sum":
                st[1][k] = cur + v
            elif a["agg"] == "min":
                st[1][k] = min(cur, v)
            elif a["agg"] == "max":
                st[1][k] = max(cur, v)
    if not gb and not acc:
        return [[0 if a["agg"] in ("count_star", "count") else None
                 for a in aggs]]
    rows = []
    for key in sorted(acc, key=lambda k: tuple(
            (1, b"") if v is None else (0, v) for v in k)):
        st = acc[key]
        row = [_out(v) for v in key]
        for k, a in enumerate(aggs):
            if a["agg"] == "count_star":
                row.append(st[0])
            elif a["agg"] == "count":
                row.append(st[2][k])
            else:
                row.append(st[1][k])
        rows.append(row)
    return rows
