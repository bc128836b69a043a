"""General LIKE / ILIKE patterns (like / not_like / ilike / not_ilike), host
side: the plain-Python reference of tests/like_common.py against `re`, the
shared C++ matcher (csrc/like.h through gpuq_test_like_match) against the
reference, the ABI values, plan-build errors and canonicalisation through the
native and the Python planner (GPUQ_FAKE_DEVICE — plan building is pure host
work), the no-pruning rule, and the staging reader."""

import os
import random
import re

import pytest

from tests import like_common as lc
from tests import strpred_common as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT = [{"agg": "count_star"}]


@pytest.fixture(scope="module", autouse=True)
def fake_device():
    os.environ["GPUQ_FAKE_DEVICE"] = "1"
    yield
    os.environ.pop("GPUQ_FAKE_DEVICE", None)


@pytest.fixture(scope="module")
def c6(tmp_path_factory):
    from datagen.gen import gen_stream

    td = tmp_path_factory.mktemp("like_cpu_c6")
    info = gen_stream(str(td), "s", "c6", **sc.GEN)
    info["data"] = sc.load(info["files"])
    return info


@pytest.fixture(scope="module")
def provider(c6):
    from parseable_amd import GpuSession, StandardTableProvider

    return StandardTableProvider(c6["stream_dir"], GpuSession())


# ---- reference vs re -------------------------------------------------------

# 1-, 2- and 3-byte characters, both ASCII cases, the three metacharacters
ALPHABET = ["a", "b", "A", "é", "日", "=", "%", "_", "\\"]
VALUE_ALPHABET = ["a", "b", "A", "B", "é", "日", "=", "%", "_", "\\"]
N_PAIRS = 24_000


def _ascii_lower(s):
    return "".join(c.lower() if "A" <= c <= "Z" else c for c in s)


def _to_regex(pat: str, fold: bool):
    """SQL pattern -> regex over str, or None for a lone trailing backslash."""
    out, i = [], 0
    while i < len(pat):
        c = pat[i]
        i += 1
        if c == "\\":
            if i >= len(pat):
                return None
            c = pat[i]
            i += 1
        elif c == "%":
            out.append(".*")
            continue
        elif c == "_":
            out.append(".")
            continue
        out.append(re.escape(_ascii_lower(c) if fold else c))
    return re.compile("".join(out), re.S)


def random_pairs(n=N_PAIRS, seed=7):
    rng = random.Random(seed)
    out = []
    for k in range(n):
        # wildcard-heavy short patterns against short values keep both the
        # match and the mismatch outcome frequent
        val = "".join(rng.choice(VALUE_ALPHABET)
                      for _ in range(rng.randint(0, 8)))
        if k % 2:
            pat = "".join(rng.choice(ALPHABET) for _ in range(rng.randint(0, 6)))
        else:
            # derived from the value, so that matches and near misses are as
            # frequent as plain mismatches: keep (escaping a metacharacter),
            # '_', '%' over a run, or a wrong character
            pat, i = "", 0
            while i < len(val):
                r = rng.random()
                if r < 0.45:
                    pat += ("\\" if val[i] in "%_\\" else "") + val[i]
                elif r < 0.65:
                    pat += "_"
                elif r < 0.9:
                    pat += "%"
                    i += rng.randint(0, 3) - 1
                else:
                    pat += rng.choice(ALPHABET)
                i += 1
        out.append((pat, val, k % 3 == 0))
    return out


@pytest.fixture(scope="module")
def pairs():
    return random_pairs()


def test_reference_matches_re(pairs):
    n_match = n_err = 0
    for pat, val, fold in pairs:
        rx = _to_regex(pat, fold)
        non_ascii = fold and any(ord(c) >= 0x80 for c in _literals(pat))
        try:
            got = lc.like(pat, val.encode(), fold)
        except lc.PatternError:
            assert rx is None or non_ascii, (pat, fold)
            n_err += 1
            continue
        assert rx is not None and not non_ascii, (pat, fold)
        want = rx.fullmatch(_ascii_lower(val) if fold else val) is not None
        assert got == want, (pat, val, fold, got, want)
        n_match += got
    # the sample exercises all three outcomes
    assert n_match > 2000 and n_err > 500 and len(pairs) - n_match - n_err > 2000


def _literals(pat):
    """Literal characters of a pattern (escape resolved, wildcards dropped)."""
    out, i = [], 0
    while i < len(pat):
        c = pat[i]
        i += 1
        if c == "\\":
            if i < len(pat):
                out.append(pat[i])
            i += 1
        elif c not in "%_":
            out.append(c)
    return out


FOUR_BYTE = [
    ("_", "😀", True), ("__", "😀", False), ("a_b", "a😀b", True),
    ("%_", "ab😀", True), ("%_b", "😀b", True), ("%😀_", "a😀é", True),
    ("_%_", "😀", False), ("_%_", "😀日", True), ("%a_%_b", "a😀b", False),
    ("😀", "😀", True), ("%\\😀", "x😀", True),
]


@pytest.mark.parametrize("pat,val,want", FOUR_BYTE)
def test_four_byte_characters(pat, val, want):
    from parseable_amd import _lib

    assert (_to_regex(pat, False).fullmatch(val) is not None) == want
    assert lc.like(pat, val.encode()) == want
    assert _lib.like_match(pat.encode(), False, val.encode()) == int(want)


def test_reference_semantics_corners():
    assert lc.like("", b"") and not lc.like("", b"a")
    assert lc.like("abc", b"abc") and not lc.like("abc", b"abcd")
    assert lc.like("%", b"") and lc.like("%%%", b"x")
    assert lc.like("a\\%", b"a%") and not lc.like("a\\%", b"ab")
    assert lc.like("\\a\\_", b"a_") and not lc.like("\\a\\_", b"ab")
    assert lc.like("a\\\\", b"a\\")
    assert lc.like("E_R", b"eXr", fold=True) and not lc.like("E_R", b"eXr")
    # haystack bytes >= 0x80 are never folded: 'É' stays distinct from 'é'
    assert not lc.like("%_", b"", fold=True)
    assert lc.like("caf_", "cafÉ".encode(), fold=True)
    # '_' on arbitrary bytes: one byte plus the continuation bytes after it
    assert lc.like("_", b"\xff\x80\x80") and not lc.like("_", b"\xff\xff")
    assert lc.like("_", b"\x80\x80") and lc.like("%_", b"a\x80")


# ---- shared C++ matcher vs reference ---------------------------------------

def test_native_matcher_random_pairs(pairs):
    from parseable_amd import _lib

    for pat, val, fold in pairs:
        try:
            want = int(lc.like(pat, val.encode(), fold))
        except lc.PatternError:
            want = -1
        got = _lib.like_match(pat.encode(), fold, val.encode())
        assert got == want, (pat, val, fold, got, want)


def test_native_matcher_arbitrary_bytes():
    """Not UTF-8: the two matchers still agree byte for byte."""
    from parseable_amd import _lib

    rng = random.Random(11)
    pool = [0x61, 0x41, 0x80, 0xBF, 0xC3, 0xE6, 0xFF, 0x25, 0x5F, 0x5C, 0x00]
    for _ in range(6000):
        pat = bytes(rng.choice(pool[:-1]) for _ in range(rng.randint(0, 6)))
        val = bytes(rng.choice(pool) for _ in range(rng.randint(0, 8)))
        try:
            want = int(lc.like(pat, val, False))
        except lc.PatternError:
            want = -1
        assert _lib.like_match(pat, False, val) == want, (pat, val)


def test_native_matcher_c6_values(c6):
    """Every pattern of the GPU lists against the distinct c6 values: the
    longest ones (the 40,000-byte message, the dense '=' run) plus a seeded
    sample."""
    from parseable_amd import _lib

    rng = random.Random(3)
    vals = []
    for col in ("message", "level", "tag"):
        d = sorted({v for v in c6["data"][col] if v is not None},
                   key=lambda v: (-len(v), v))
        vals += d[:40] + rng.sample(d[40:], min(len(d[40:]), 600))
    assert max(len(v) for v in vals) == 40_000
    for pat in lc.all_fixed_patterns() + lc.random_patterns():
        for fold in (False, True):
            try:
                segs = lc.compile_pattern(pat.encode(), fold)
            except lc.PatternError:
                assert _lib.like_match(pat.encode(), fold, b"x") == -1
                continue
            for v in vals:
                want = lc.match_compiled(segs, lc._lower(v) if fold else v)
                assert _lib.like_match(pat.encode(), fold, v) == int(want), (
                    pat, fold, v[:80])


# ---- ABI and errors --------------------------------------------------------

def test_op_values():
    from parseable_amd import _lib

    assert [_lib.OPS[o] for o in lc.PATTERN_OPS] == [17, 18, 19, 20]
    assert _lib.OPS["is_not_null"] == 16
    assert tuple(lc.PATTERN_OPS) == _lib.PATTERN_OPS
    src = open(os.path.join(ROOT, "include", "gpuq.h")).read()
    assert re.search(r"GPUQ_LIKE = 17,\s*GPUQ_NOT_LIKE,\s*GPUQ_ILIKE,\s*"
                     r"GPUQ_NOT_ILIKE\s*\} gpuq_op;", src)


def _scan(provider, q, native):
    if native:
        os.environ.pop("GPUQ_PY_PLANNER", None)
    else:
        os.environ["GPUQ_PY_PLANNER"] = "1"
    try:
        return provider.scan(dict(q))
    finally:
        os.environ.pop("GPUQ_PY_PLANNER", None)


def _build_error(provider, pred, native):
    from parseable_amd.provider import GpuqError

    with pytest.raises(GpuqError) as ei:
        _scan(provider, {"select": COUNT, "preds": [pred]}, native)
    return str(ei.value)


@pytest.mark.parametrize("native", [True, False])
def test_plan_build_errors(provider, native):
    def err(col, op, lit):
        return _build_error(provider, {"col": col, "op": op, "lit": lit}, native)

    for op in lc.PATTERN_OPS:
        assert f"{op} pattern ends in a lone backslash: message" in err(
            "message", op, "abc\\")
        assert f"{op} pattern has more than 255 elements: message" in err(
            "message", op, "%" + "a" * 256)
        assert f"{op} pattern has more than 16 %-separated segments" in err(
            "message", op, "%".join("abcdefghijklmnopq"))
        assert f"string predicate {op} on non-utf8 column: latency" in err(
            "latency", op, "1%")
        assert f"{op} needs a string literal: message" in err("message", op, 5)
    assert "ilike literal must be ASCII" in err("message", "ilike", "caf_é%")
    assert "not_ilike literal must be ASCII" in err("message", "not_ilike", "É")
    # the limits themselves build: 255 elements, 16 segments
    for lit in ("%" + "a" * 255, "%".join("abcdefghijklmnop"),
                "%" + "%".join("abcdefghijklmn") + "%"):
        _scan(provider, {"select": COUNT, "preds": [
            {"col": "message", "op": "like", "lit": lit}]}, native).close()
    # like (no folding) takes a non-ASCII literal
    _scan(provider, {"select": COUNT, "preds": [
        {"col": "message", "op": "like", "lit": "caf_é%"}]}, native).close()


# ---- canonicalisation ------------------------------------------------------

def _plan(provider, preds, native, capfd):
    """-> ([(op, path, as or None)], (rows_scanned, bytes_scanned))"""
    os.environ["GPUQ_PLAN_DEBUG"] = "1"
    try:
        capfd.readouterr()
        plan = _scan(provider, {"select": COUNT, "preds": preds}, native)
        m = plan.metrics()
        plan.close()
        err = capfd.readouterr().err
    finally:
        os.environ.pop("GPUQ_PLAN_DEBUG", None)
    lines = re.findall(
        r"\[gpuq plan\] pred \d+ col=\S+ op=(\S+) path=(\S+)(?: as=(\S+))?\n",
        err)
    return ([(o, p, a or None) for o, p, a in lines],
            (m["rows_scanned"], m["bytes_scanned"]))


CANON = [
    ("like", "%error%", "contains", "error"),
    ("not_like", "%error%", "not_contains", "error"),
    ("ilike", "%ErRor%", "icontains", "error"),
    ("not_ilike", "%ERROR%", "not_icontains", "error"),
    ("like", "Error%", "starts_with", "Error"),
    ("not_like", "Error%", "not_starts_with", "Error"),
    ("like", "%TIMEOUT", "ends_with", "TIMEOUT"),
    ("not_like", "%TIMEOUT", "not_ends_with", "TIMEOUT"),
    ("like", "%%100\\%%", "contains", "100%"),
    ("like", "a\\_b%%", "starts_with", "a_b"),
    ("like", "%", "contains", ""),
    ("not_like", "%%%", "not_contains", ""),
    ("ilike", "%", "contains", ""),
    ("not_ilike", "%%", "not_contains", ""),
]


@pytest.mark.parametrize("native", [True, False])
@pytest.mark.parametrize("op,pat,as_op,lit", CANON)
def test_canonical_shapes_build_the_existing_plan(provider, capfd, native, op,
                                                  pat, as_op, lit):
    got, m = _plan(provider, [{"col": "message", "op": op, "lit": pat}],
                   native, capfd)
    assert got == [(op, "lut+window", as_op)], got
    want, m0 = _plan(provider, [{"col": "message", "op": as_op, "lit": lit}],
                     native, capfd)
    assert want == [(as_op, "lut+window", None)], want
    assert m == m0


@pytest.mark.parametrize("native", [True, False])
@pytest.mark.parametrize("op,pat", [
    ("like", "a%b"), ("like", "%a_"), ("like", "abc"), ("ilike", "abc%"),
    ("ilike", "%abc"), ("not_ilike", "abc"), ("like", ""), ("like", "%a_b%"),
    ("not_like", "_%"), ("like", "a\\%"),
])
def test_general_patterns_are_not_rewritten(provider, capfd, native, op, pat):
    got, _ = _plan(provider, [{"col": "message", "op": op, "lit": pat}],
                   native, capfd)
    assert got == [(op, "lut+window", None)], got
    # dict-only column: LUT alone; a no-wildcard pattern does not force hash
    got, _ = _plan(provider, [{"col": "level", "op": op, "lit": pat}],
                   native, capfd)
    assert got == [(op, "lut", None)], got


# ---- no pruning ------------------------------------------------------------

@pytest.mark.parametrize("op", lc.PATTERN_OPS)
@pytest.mark.parametrize("col,pat", [
    ("message", "ZZZ%"), ("level", "zzzz_%x"), ("level", "!%_"), ("tag", "ZZZ%"),
    ("tag", "!"),
])
def test_patterns_never_prune(provider, op, col, pat):
    """A pattern outside every file's [min, max] of the column scans the row
    groups a predicate-free query scans, in both planners."""
    sel = [{"agg": "max", "col": "latency"}]   # not a manifest-answered count

    def stats(preds, native):
        plan = _scan(provider, {"select": sel, "preds": preds}, native)
        try:
            m = plan.metrics()
            return m["rows_scanned"], m["rowgroup_bytes_total"]
        finally:
            plan.close()

    base = stats([], True)
    assert base[0] == sc.GEN["rows"]
    for native in (True, False):
        assert stats([{"col": col, "op": op, "lit": pat}], native) == base


# ---- seeded random patterns ------------------------------------------------

def test_random_patterns_split_the_message_column(c6):
    pats = lc.random_patterns()
    assert len(pats) == lc.N_RANDOM and len(set(pats)) == len(pats)
    assert pats == lc.random_patterns()   # deterministic
    data = c6["data"]
    non_null = sum(v is not None for v in data["message"])
    assert non_null == lc.NON_NULL["message"]
    split = sum(0 < lc.count(data, "message", "like", p) < non_null
                for p in pats)
    assert 2 * split >= len(pats), split


def test_reference_counts_of_the_fixed_lists(c6):
    """The counts the GPU test asserts, from the reference alone."""
    data = c6["data"]
    for col in lc.NON_NULL:
        assert sum(v is not None for v in data[col]) == lc.NON_NULL[col]
    lists = [("message", lc.MESSAGE_PATTERNS + lc.DENSE_PATTERNS),
             ("level", lc.LEVEL_PATTERNS), ("tag", lc.TAG_PATTERNS)]
    for col, lst in lists:
        for pat, n_like, n_ilike in lst:
            assert lc.count(data, col, "like", pat) == n_like, (col, pat)
            assert lc.count(data, col, "not_like", pat) == \
                lc.NON_NULL[col] - n_like
            if n_ilike is not None:
                assert lc.count(data, col, "ilike", pat) == n_ilike, (col, pat)
    for pat, n in lc.MESSAGE_VACUOUS + lc.MULTIBYTE_PATTERNS:
        assert lc.count(data, "message", "like", pat) == n, pat
    big = [i for i, v in enumerate(data["message"]) if v and len(v) == 40_000]
    assert len(big) == 1
    for pat in lc.BIG_PATTERNS:
        q = {"preds": [{"col": "message", "op": "like", "lit": pat}]}
        assert lc.selected(data, q) == big, pat


# ---- staging leg -----------------------------------------------------------

STAGE_START = 10_000


@pytest.fixture(scope="module")
def staged(tmp_path_factory):
    """A staging-only stream (empty manifest list, .arrows files alone): every
    row is read by StagingScanner on the host."""
    import json

    import pyarrow as pa

    from datagen.gen import gen_staging

    td = tmp_path_factory.mktemp("like_staging")
    sdir = str(td / "s")
    os.makedirs(sdir)
    with open(os.path.join(sdir, "stream.json"), "w") as fh:
        json.dump({"version": "v6", "objectstore-format": "v6",
                   "stream_type": "UserDefined",
                   "snapshot": {"version": "v2", "manifest_list": []}}, fh)
    stg = str(td / "staging")
    st = gen_staging(stg, config="c6", rows=6_000, n_arrows=2, n_parquet=0,
                     start_minute=STAGE_START)
    data = {}
    for p in st["arrows"]:
        with pa.ipc.open_stream(p) as r:
            t = r.read_all()
        for name in t.column_names:
            c = t.column(name)
            if pa.types.is_string(c.type):
                c = c.cast(pa.binary())
            elif pa.types.is_timestamp(c.type):
                c = c.cast(pa.int64())
            data.setdefault(name, []).extend(c.to_pylist())
    return sdir, stg, st, data


STAGE_CASES = (
    [("message", p) for p in ("%_rror", "Err_r%", "E%r", "%é%É%", "%caf_ %",
                              "%日_ %", "%r%r%r%", "_", "", "%_", "%", "abc",
                              "Error", "%\\%%", "%a_b%")]
    + [("level", p) for p in ("E%R", "_rror", "W__N", "%e_u%", "_____")]
)


@pytest.mark.parametrize("op", lc.PATTERN_OPS)
def test_staging_leg(staged, op):
    from oracle.compare import assert_rows_equal
    from parseable_amd import Query, StandardTableProvider
    from parseable_amd.provider import GpuqError

    sdir, stg, st, data = staged
    prov = StandardTableProvider(sdir, None, staging_dir=stg,
                                 now_ms=st["max_ts"])
    n_split = 0
    for col, pat in STAGE_CASES:
        q = {"select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"}],
             "group_by": ["level"],
             "preds": [{"col": col, "op": op, "lit": pat}]}
        if op.endswith("ilike") and not pat.isascii():
            with pytest.raises(GpuqError, match="literal must be ASCII"):
                Query(prov).execute(dict(q))
            continue
        rows, _ = Query(prov).execute(dict(q))
        assert_rows_equal(rows, lc.expected(data, q), f"staging {op} {pat!r}")
        n_sel = len(lc.selected(data, q))
        n_split += 0 < n_sel < sum(v is not None for v in data[col])
    assert n_split >= 10, n_split
    for bad, msg in (("x\\", "lone backslash"), ("a" * 256, "255 elements"),
                     ("%".join("abcdefghijklmnopq"), "16 %-separated")):
        with pytest.raises(GpuqError, match=msg):
            Query(prov).execute({"select": COUNT, "preds": [
                {"col": "message", "op": op, "lit": bad}]})
