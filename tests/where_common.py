"""Expected values for the WHERE-tree tests (`query["where"]`: nested
{"and": [...]} / {"or": [...]} groups over leaf preds), computed in plain
Python over the parquet files read with pyarrow — the oracle does not know
trees, so the tests carry their own reference, in the manner of
tests/strpred_common.py (whose loader, constants and LIKE / null leaf rules
are reused).

Semantics (include/gpuq.h): a leaf is False on a NULL row, is_null alone
excepted; groups combine those booleans; `preds`, `time_range` and `where`
are AND-ed at the root. Row shaping follows strpred_common.expected, plus avg
(sum / count, None over no value) and count_distinct."""

import random

from tests import strpred_common as sc

BASE, MIN, GEN = sc.BASE, sc.MIN, sc.GEN
# second stream: partitions and row ranges that are no multiple of 16
GEN_ODD = dict(rows=1003, rows_per_file=400, data_page_size=65536)

load = sc.load


def group_kind(node):
    if "and" in node:
        return "and"
    if "or" in node:
        return "or"
    return None


def match(p, v):
    """One leaf against one value (utf8 as bytes)."""
    op = p["op"]
    if op in ("eq", "ne", "lt", "le", "gt", "ge"):
        if v is None:
            return False
        lit = p["lit"].encode() if isinstance(p["lit"], str) else p["lit"]
        return {"eq": v == lit, "ne": v != lit, "lt": v < lit, "le": v <= lit,
                "gt": v > lit, "ge": v >= lit}[op]
    return sc.match(p, v)


def leaves(node):
    k = group_kind(node)
    if k is None:
        return [node]
    return [x for kid in node[k] for x in leaves(kid)]


def node_rows(data, node):
    """-> set of row indices satisfying the (sub)tree."""
    k = group_kind(node)
    if k is None:
        col = data[node["col"]]
        return {i for i in range(len(col)) if match(node, col[i])}
    sets = [node_rows(data, kid) for kid in node[k]]
    out = sets[0]
    for s in sets[1:]:
        out = out & s if k == "and" else out | s
    return out


def root_node(query):
    kids = list(query.get("preds", []))
    tr = query.get("time_range")
    if tr:
        kids.append({"col": "p_timestamp", "op": "between", "lo": tr[0],
                     "hi": tr[1], "hi_exclusive": True})
    if query.get("where") is not None:
        kids.append(query["where"])
    return kids


def selected(data, query):
    """Sorted row indices satisfying preds AND time_range AND where."""
    rows = set(range(len(data["p_timestamp"])))
    for kid in root_node(query):
        rows &= node_rows(data, kid)
    return sorted(rows)


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
            if a["agg"] == "count_distinct":
                st[1][k] = (cur or set()) | {v}
            elif cur is None:
                st[1][k] = v
            elif a["agg"] in ("sum", "avg"):
                st[1][k] = cur + v
            elif a["agg"] == "min":
                st[1][k] = min(cur, v)
            elif a["agg"] == "max":
                st[1][k] = max(cur, v)

    def final(a, st, k):
        if a["agg"] == "count_star":
            return st[0]
        if a["agg"] == "count":
            return st[2][k]
        if a["agg"] == "count_distinct":
            return len(st[1][k] or ())
        if a["agg"] == "avg":
            return st[1][k] / st[2][k] if st[2][k] else None
        return st[1][k]

    if not gb and not acc:
        return [[0 if a["agg"] in ("count_star", "count", "count_distinct")
                 else None for a in aggs]]
    rows = []
    for key in sorted(acc, key=lambda k: tuple(
            (1, b"") if v is None else (0, v) for v in k)):
        st = acc[key]
        rows.append([_out(v) for v in key]
                    + [final(a, st, k) for k, a in enumerate(aggs)])
    return rows


# ---- leaf pool: one entry per evaluation path -----------------------------
# path -> (leaf builder over a literal choice, extra query keys). The GPU
# tests read the path a leaf really took from the plan-debug lines.

def leaf(col, op, lit=None, **kw):
    p = {"col": col, "op": op}
    if lit is not None:
        p["lit"] = lit
    p.update(kw)
    return p


def ts_between(lo_ms, hi_ms):
    return {"col": "p_timestamp", "op": "between", "lo": BASE + lo_ms,
            "hi": BASE + hi_ms}


# c6 leaves by path. `tag` takes the hash path when it is a group key
# (query_for); the between straddles files 0|1 and 1|2 so that file 1's row
# group is proven (elided) and files 0 and 2 are boundary row groups.
POOL = {
    "lut": [leaf("level", "eq", "ERROR"), leaf("level", "starts_with", "W"),
            leaf("level", "not_icontains", "o"), leaf("level", "ge", "info")],
    "lut+window": [leaf("message", "contains", "TIMEOUT"),
                   leaf("message", "icontains", "error"),
                   leaf("message", "ends_with", "r"),
                   leaf("message", "not_contains", "e")],
    "hash": [leaf("tag", "contains", "ag-0001"), leaf("tag", "eq", "Tag-000007"),
             leaf("tag", "not_ends_with", "7"), leaf("tag", "lt", "TAG-000100")],
    "i64": [leaf("latency", "lt", 100_000), leaf("latency", "ge", 900_000),
            leaf("opt_i64", "gt", 500_000_000), leaf("latency", "ne", 5)],
    "f64": [leaf("f_f64", "lt", 0.25), leaf("f_f64", "ge", 0.9),
            leaf("f_f64", "gt", 0.5), leaf("f_f64", "ne", 0.125)],
    "between": [ts_between(40_000, 140_000), ts_between(100_000, 170_000)],
    "nulltask": [leaf("message", "is_null"), leaf("opt_i64", "is_null"),
                 leaf("tag", "is_not_null"), leaf("level", "is_null")],
}
PATHS = list(POOL)


def needs_hash(node):
    return any(x["col"] == "tag" and x["op"] not in sc.NULL_OPS
               for x in leaves(node))


def query_for(node, select=None):
    """A count query over the tree; `tag` leaves ride the hash path through a
    GROUP BY tag (a column with PLAIN pages used as a key)."""
    q = {"select": select or [{"agg": "count_star"}], "where": node}
    if needs_hash(node):
        q["group_by"] = ["tag"]
    return q


def leaf_path(p):
    for path, pool in POOL.items():
        if any(p is x or p == x for x in pool):
            return path
    raise KeyError(p)


def random_trees(data, seed=20240607, want=48, max_leaves=6, max_depth=3):
    """Seeded random trees over POOL, kept only when the reference selects
    some but not all rows — no executed case is vacuous. -> [(tree, n_sel)]"""
    rng = random.Random(seed)
    n_all = len(data["p_timestamp"])
    cache = {}

    def rows_of(p):
        key = repr(p)
        if key not in cache:
            cache[key] = frozenset(node_rows(data, p))
        return cache[key]

    def tree_rows(node):
        k = group_kind(node)
        if k is None:
            return rows_of(node)
        sets = [tree_rows(kid) for kid in node[k]]
        out = sets[0]
        for s in sets[1:]:
            out = out & s if k == "and" else out | s
        return out

    def gen(depth, budget, kind):
        """A group of `kind` with 2..budget leaves below it."""
        kids, left = [], budget
        n_kids = rng.randint(2, min(3, budget))
        for j in range(n_kids):
            rest = n_kids - j - 1
            if depth < max_depth and left - rest >= 2 and rng.random() < 0.45:
                take = rng.randint(2, left - rest)
                kids.append(gen(depth + 1, take, "or" if kind == "and" else "and"))
                left -= len(leaves(kids[-1]))
            else:
                path = rng.choice(PATHS)
                kids.append(rng.choice(POOL[path]))
                left -= 1
        return {kind: kids}

    out, tries = [], 0
    while len(out) < want and tries < 4000:
        tries += 1
        t = gen(1, rng.randint(2, max_leaves), rng.choice(["or", "or", "and"]))
        if "or" not in repr(t):
            continue
        n = len(tree_rows(t))
        if 0 < n < n_all:
            out.append((t, n))
    return out
