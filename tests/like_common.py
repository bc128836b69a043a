"""Plain-Python reference for the general LIKE / ILIKE pattern ops (like,
not_like, ilike, not_ilike — include/gpuq.h), written from the semantics and
independently of csrc/like.h:

  - '%' any byte sequence, '_' one character = one byte plus every directly
    following byte in 0x80..0xBF, backslash makes the next byte literal, a
    lone trailing backslash is an error;
  - anchored at both ends; a NULL value satisfies none of the four ops;
  - ilike folds ASCII A-Z on both sides; a literal pattern byte >= 0x80 is an
    error there;
  - at most 255 elements and 16 '%'-separated segments.

The matcher has no backtracking: first segment forward from 0, last segment
backward from the end, every middle segment at its leftmost match between the
two. test_like_cpu.py checks it against `re` on random pattern/value pairs.

Every other op is delegated to tests/strpred_common.py; `selected` and
`expected` additionally evaluate a `where` tree ({"and": [...]} /
{"or": [...]} over leaves)."""

import functools
import random

from tests import strpred_common as sc

PATTERN_OPS = ["like", "not_like", "ilike", "not_ilike"]
MAX_ELEMS, MAX_SEGS = 255, 16
ANY = -1   # the '_' element


class PatternError(ValueError):
    pass


def _lower(b: bytes) -> bytes:
    return bytes(c | 0x20 if 0x41 <= c <= 0x5A else c for c in b)


def compile_pattern(pat: bytes, fold: bool):
    """-> list of segments; a segment is a list of elements (a byte value, or
    ANY). len == 1: no '%'. The first / last segment may be empty."""
    segs = [[]]
    n_elem = 0
    it = iter(range(len(pat)))
    prev_pct = False
    for i in it:
        c = pat[i]
        if c == ord("%"):
            if not prev_pct:
                segs.append([])
                if len(segs) > MAX_SEGS:
                    raise PatternError("too many segments")
            prev_pct = True
            continue
        prev_pct = False
        if c == ord("\\"):
            j = next(it, None)
            if j is None:
                raise PatternError("trailing backslash")
            el = pat[j]
        elif c == ord("_"):
            el = ANY
        else:
            el = c
        if el != ANY and fold:
            if el >= 0x80:
                raise PatternError("non-ascii ilike literal")
            el = _lower(bytes([el]))[0]
        n_elem += 1
        if n_elem > MAX_ELEMS:
            raise PatternError("too many elements")
        segs[-1].append(el)
    return segs


def _cont(b):
    return 0x80 <= b <= 0xBF


def _forward(seg, v, pos, limit):
    """End of seg matched at pos without passing limit, or None."""
    for el in seg:
        if pos >= limit:
            return None
        if el == ANY:
            pos += 1
            while pos < limit and _cont(v[pos]):
                pos += 1
        else:
            if v[pos] != el:
                return None
            pos += 1
    return pos


def _backward(seg, v, end):
    """Start of seg matched so that it ends at `end`, or None."""
    p = end
    for el in seg[::-1]:
        if p < 1:
            return None
        if el == ANY:
            p -= 1
            while p > 0 and _cont(v[p]):
                p -= 1
        else:
            if v[p - 1] != el:
                return None
            p -= 1
    return p


def match_compiled(segs, v: bytes) -> bool:
    n = len(v)
    if len(segs) == 1:
        return _forward(segs[0], v, 0, n) == n
    pos = _forward(segs[0], v, 0, n)
    tail = _backward(segs[-1], v, n)
    if pos is None or tail is None or tail < pos:
        return False
    for seg in segs[1:-1]:
        q = pos
        while True:
            if seg[0] != ANY:   # skip starts whose first byte cannot match
                q = v.find(bytes(seg[:1]), q, tail)
            if q < 0 or q > tail:
                return False
            end = _forward(seg, v, q, tail)
            if end is not None:
                pos = end
                break
            q += 1
    return True


def like(pattern, value: bytes, fold=False) -> bool:
    if isinstance(pattern, str):
        pattern = pattern.encode()
    segs = compile_pattern(pattern, fold)
    return match_compiled(segs, _lower(value) if fold else value)


def match(p, v):
    op = p["op"]
    if op not in PATTERN_OPS:
        return sc.match(p, v)
    if v is None:
        return False
    return like(p["lit"], v, fold=op.endswith("ilike")) != op.startswith("not_")


def _matcher(p):
    """leaf -> f(value); a pattern op is compiled once and evaluated once per
    distinct value."""
    op = p["op"]
    if op not in PATTERN_OPS:
        return lambda v: sc.match(p, v)
    fold, neg = op.endswith("ilike"), op.startswith("not_")
    segs, memo = _compiled(p["lit"], fold)

    def f(v):
        if v is None:
            return False
        r = memo.get(v)
        if r is None:
            r = memo[v] = match_compiled(segs, _lower(v) if fold else v)
        return r != neg
    return f


@functools.lru_cache(maxsize=4)
def _compiled(pattern: str, fold: bool):
    """(segments, per-value result memo): an op and its negation, and the
    count and the expected rows of one case, share the matcher's work."""
    return compile_pattern(pattern.encode(), fold), {}


def tree_eval(node, row_value, cache=None):
    """A where tree ({"and": [..]} / {"or": [..]} / leaf) on one row;
    row_value(col) -> the row's value."""
    cache = {} if cache is None else cache
    for kind in ("and", "or"):
        if kind in node:
            vals = (tree_eval(k, row_value, cache) for k in node[kind])
            return all(vals) if kind == "and" else any(vals)
    f = cache.get(id(node))
    if f is None:
        f = cache[id(node)] = _matcher(node)
    return f(row_value(node["col"]))


def selected(data, query):
    """Row indices satisfying every predicate, the time range and the where
    tree."""
    conj = list(query.get("preds", []))
    tr = query.get("time_range")
    if tr:
        conj.append({"col": "p_timestamp", "op": "between", "lo": tr[0],
                     "hi": tr[1], "hi_exclusive": True})
    if query.get("where") is not None:
        conj.append(query["where"])
    cache = {}
    return [i for i in range(len(data["p_timestamp"]))
            if all(tree_eval(p, lambda c: data[c][i], cache) for p in conj)]


def expected(data, query):
    """Rows in the engine's normalized form (strpred_common.expected over the
    selected rows)."""
    idx = selected(data, query)
    sub = {k: [v[i] for i in idx] for k, v in data.items()}
    rest = {k: v for k, v in query.items()
            if k not in ("preds", "time_range", "where")}
    return sc.expected(sub, rest)


def count(data, col, op, pattern):
    f = _matcher({"col": col, "op": op, "lit": pattern})
    return sum(f(v) for v in data[col])


# ---- fixed pattern lists over the c6 fixture (strpred_common.GEN) ---------
# (pattern, like count, ilike count or None)

NON_NULL = {"message": 45_490, "level": 53_975, "tag": 42_013}

MESSAGE_PATTERNS = [
    ("%_rror", 3258, 6369), ("Err_r%", 1499, 5815), ("E%r", 1351, 2961),
    ("Error _%", 1010, 3804), ("%Zone%queue%", 7628, None),
    ("%é%É%", 17208, None), ("%r%r%r%", 31374, None),
    ("%e%r%r%o%r%", 24842, None), ("%a_b%", 1252, None), ("_", 791, None),
    ("__", 1898, None), ("___%", 41479, None), ("%_", 44168, None),
    ("", 1322, None),
]
# all-or-none cases, asserted by value
MESSAGE_VACUOUS = [("%\\%%", 0), ("%ZZZabsentQQ%x%", 0), ("%", 45_490)]
MULTIBYTE_PATTERNS = [("%caf_ %", 18793), ("%日_ %", 18761)]
DENSE_PATTERNS = [("%=%=error", 64, 128), ("=%_rror", 128, None),
                  ("%====%Error", 64, 128)]
BIG_PATTERNS = ["Error%TIMEOUT", "%rror%TIMEOUT%", "%Error %x%TIMEOUT"]
LEVEL_PATTERNS = [
    ("E%R", 4432, 13374), ("_rror", 8942, 13374), ("W__N", 4537, 13589),
    ("%e_u%", 8981, 13460), ("D_bug", 4461, 13460), ("_____", 26834, None),
]
TAG_PATTERNS = [
    ("Tag-%7", 1316, 4107), ("tag-0000_1", 289, 872), ("T%-0001__", 5485, 8186),
    ("___-000007", 94, None), ("%g-0%9", 2907, None),
]


def all_fixed_patterns():
    out = [p for p, *_ in MESSAGE_PATTERNS + LEVEL_PATTERNS + TAG_PATTERNS
           + DENSE_PATTERNS]
    out += [p for p, _ in MESSAGE_VACUOUS + MULTIBYTE_PATTERNS]
    return out + BIG_PATTERNS


# ---- seeded random patterns over c6 ---------------------------------------

RANDOM_SEED = 20260
N_RANDOM = 40


def random_patterns(n=N_RANDOM, seed=RANDOM_SEED):
    """Patterns built from pieces of the c6 vocabulary joined and wrapped by
    '%', with characters replaced by '_' and ASCII case flipped at random.
    Deterministic; shared by the CPU and the GPU test."""
    from datagen.gen import C6_TOKENS, C6_WORDS

    rng = random.Random(seed)
    vocab = C6_TOKENS + C6_WORDS

    def piece():
        w = list(vocab[rng.randrange(len(vocab))])   # characters, not bytes
        if len(w) > 2 and rng.random() < 0.4:
            a = rng.randrange(len(w) - 1)
            w = w[a:a + rng.randint(2, len(w) - a)]
        if rng.random() < 0.35:
            w[rng.randrange(len(w))] = "_"
        if rng.random() < 0.2:
            k = rng.randrange(len(w))
            w[k] = w[k].swapcase() if w[k].isascii() else w[k]
        return "".join(w)

    out = []
    while len(out) < n:
        parts = [piece() for _ in range(rng.choice((1, 1, 2, 2, 3)))]
        if rng.random() < 0.3:
            parts.insert(rng.randrange(len(parts) + 1), " ")
        pat = "%".join(parts)
        if rng.random() < 0.8:
            pat = "%" + pat
        if rng.random() < 0.8:
            pat = pat + "%"
        if pat not in out:
            out.append(pat)
    return out
