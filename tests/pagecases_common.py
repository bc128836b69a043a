"""Parquet page-decode edge cases: fixture writers, a page inspector and a
plain-Python query reference over the source arrays.

Every GPU test elsewhere reaches the page decoders through datagen streams,
which cover a narrow part of what the decoders accept (small delta widths,
a handful of dictionary index widths, i.i.d. nulls, nullable columns only,
no INT32). The writers here use pyarrow alone to produce small files whose
pages have the shapes those streams never have; the inspector reads the same
files back without pyarrow's decoders (own Thrift-compact PageHeader reader,
pa.Codec for decompression only, arbitrary-precision Python ints for every
bit field) so that tests/test_pagecases_cpu.py can prove each file contains
the shape it claims, and tests/test_gpu_pagecases.py can compare the device
decoders against the source arrays the files were written from.

A case is a `Case`: the file path, the row count and `cols`, the source
column values as object arrays (None = NULL) in file row order. Every file
holds one row group, data page v1, and a unique p_timestamp (strictly
decreasing in file order unless stated), so a full projection has a defined
row order: file order.
"""

from __future__ import annotations

import os
import struct
from dataclasses import dataclass, field

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

I64_MIN, I64_MAX = -(2**63), 2**63 - 1
I32_MIN, I32_MAX = -(2**31), 2**31 - 1
TS0 = 1756684800000

DELTA_WIDTHS = (1, 7, 8, 9, 31, 32, 33, 56, 57, 58, 59, 60, 61, 62, 63, 64)
DELTA_HARD_WIDTHS = (59, 61, 62, 63)   # a 64-bit bit-reader accumulator spills
DELTA_EXTRA = ("const", "dec", "alt")
DELTA_ROWS = (1, 2, 64, 65, 256, 257, 1000)
DELTA_MP_ROWS = 5000
DICT_SIZES_SMALL = (1, 2, 3, 4, 5, 8, 9, 255, 256, 257, 511, 513, 4095, 4097)
DICT_SIZES_BIG = (65535, 65537)
DICT_INDEX_WIDTHS = (0, 1, 2, 3, 4, 8, 9, 12, 13, 16, 17)
DICT_TYPES = ("i64", "f64", "str")
DICT_ROWS_SMALL = 9000
DICT_ROWS_BIG = 70000
VARIANTS = ("req", "nn", "nul")   # required / nullable null-free / with nulls
DEF_LAYOUTS = ("all_null", "all_valid", "null_first", "null_last", "alt", "runs")
DEF_RUN_LENGTHS = (1, 7, 8, 9, 63, 64, 65, 1000)
DEF_ROWS = 2507                    # not a multiple of 8
INT32_KINDS = ("dict", "plain", "delta")
INT32_ROWS = 3000
MP_BATCH = 999                     # page row count of the multi-page files
KEYS = ("k0", "k1", "k2", "k3", "k4")


@dataclass
class Case:
    name: str
    path: str
    n: int
    cols: dict = field(default_factory=dict)   # name -> object ndarray


# ---------------------------------------------------------------------------
# writers
# ---------------------------------------------------------------------------

def _obj(values):
    a = np.empty(len(values), dtype=object)
    for i, v in enumerate(values):
        a[i] = v
    return a


def _null_mask(n, rng, p=0.25):
    """True = valid. Random nulls at rate p plus one long null run and one
    long valid run, so def levels mix RLE and bit-packed runs."""
    m = rng.random(n) >= p
    if n >= 80:
        m[10:31] = False
        m[37:80] = True
    if n >= 2:
        m[0] = True       # keep at least one value
        m[n - 1] = False  # and at least one null
    return m


def _with_nulls(values, mask):
    """None where the mask is False; elsewhere the dense prefix of values in
    order. A page stores only the present values, so the dense stream keeps
    the shape (delta widths, dictionary size, run lengths) values was built
    with instead of losing a random quarter of it."""
    it = iter(values)
    return [next(it) if ok else None for ok in mask]


class _Spec:
    """Columns of one file, in order."""

    def __init__(self, n, ts=None, ts_enc="plain"):
        self.n = n
        self.fields, self.arrays, self.src = [], [], {}
        self.dict_cols, self.enc = [], {}
        if ts is None:
            ts = [TS0 + 7 * (n - 1 - i) for i in range(n)]
        self.add("p_timestamp", pa.timestamp("ms"), ts, True, ts_enc)

    def add(self, name, typ, values, nullable, enc):
        assert len(values) == self.n and name not in self.src
        self.fields.append(pa.field(name, typ, nullable=nullable))
        self.arrays.append(pa.array(values, type=typ))
        self.src[name] = _obj(values)
        if enc == "dict":
            self.dict_cols.append(name)
        elif enc == "delta":
            self.enc[name] = "DELTA_BINARY_PACKED"
        else:
            self.enc[name] = "PLAIN"

    def add_variants(self, stem, typ, values, enc, rng):
        """stem_req / stem_nn / stem_nul"""
        self.add(f"{stem}_req", typ, list(values), False, enc)
        self.add(f"{stem}_nn", typ, list(values), True, enc)
        self.add(f"{stem}_nul", typ,
                 _with_nulls(values, _null_mask(self.n, rng)), True, enc)

    def add_key_and_other(self, rng):
        """k: small utf8 group key; o: an INT64 PLAIN 'other' column."""
        self.add("k", pa.string(),
                 [KEYS[int(x)] for x in rng.integers(0, len(KEYS), self.n)],
                 True, "dict")
        self.add("o", pa.int64(),
                 [int(x) for x in rng.integers(-1000, 1000, self.n)],
                 True, "plain")

    def write(self, name, out_dir, compression="lz4", multipage=False,
              dict_limit=64 << 20):
        path = os.path.join(out_dir, f"{name}.parquet")
        tbl = pa.Table.from_arrays(self.arrays, schema=pa.schema(self.fields))
        kw = {}
        if multipage:
            # the writer closes a page once a batch leaves it above
            # data_page_size: every batch becomes a page of MP_BATCH rows
            kw = dict(data_page_size=16, write_batch_size=MP_BATCH)
        pq.write_table(tbl, path, row_group_size=1 << 20,
                       compression=compression,
                       use_dictionary=list(self.dict_cols),
                       column_encoding=dict(self.enc),
                       data_page_version="1.0", write_statistics=True,
                       dictionary_pagesize_limit=dict_limit, **kw)
        return Case(name, path, self.n, self.src)


def _delta_values(b, n, rng):
    """Values whose miniblocks need exactly b bits: integers(0, 2**(b-1))
    gives deltas spanning just under 2**b. b == 1 needs deltas in {0, 1}
    (a random non-decreasing walk: integers(0, 1) would be constant), b ==
    64 the full int64 range with both extremes."""
    if b == 1:
        return [int(x) for x in np.cumsum(rng.integers(0, 2, n))]
    if b == 64:
        v = [int(x) for x in rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64,
                                          endpoint=True)]
        for i, x in enumerate((I64_MAX, I64_MIN, -1, 0, I64_MIN, I64_MAX)):
            if i < n:
                v[i] = x
        return v
    return [int(x) for x in rng.integers(0, 2 ** (b - 1), n, dtype=np.int64)]


def _delta_extra(kind, n, rng):
    if kind == "const":
        return [123456789012] * n
    if kind == "dec":     # strictly decreasing: every delta negative
        steps = rng.integers(1, 1000, n)
        return [10**15 - int(x) for x in np.cumsum(steps)]
    return [I64_MIN if i % 2 else I64_MAX for i in range(n)]   # "alt": wraps


def delta_case(out_dir, n, compression="lz4", multipage=False, tag=None):
    """d_<b>_<variant> for b in DELTA_WIDTHS, d_<extra>_<variant> for
    DELTA_EXTRA; all INT64 DELTA_BINARY_PACKED."""
    rng = np.random.default_rng(1000 + n)
    sp = _Spec(n)
    sp.add_key_and_other(rng)
    for b in DELTA_WIDTHS:
        sp.add_variants(f"d_{b}", pa.int64(), _delta_values(b, n, rng),
                        "delta", rng)
    for kind in DELTA_EXTRA:
        sp.add_variants(f"d_{kind}", pa.int64(), _delta_extra(kind, n, rng),
                        "delta", rng)
    name = tag or (f"delta_mp_{n}" if multipage else f"delta_{n}")
    return sp.write(name, out_dir, compression, multipage)


def delta_ts_case(out_dir, n=3000):
    """p_timestamp itself delta-encoded and far from monotone: unique
    10-minute slots in shuffled order, so neighbouring rows lie hours apart
    in either direction. `v` is the file row index."""
    rng = np.random.default_rng(77)
    ts = [TS0 + 600_000 * int(x) for x in rng.permutation(n)]
    sp = _Spec(n, ts, "delta")
    sp.add_key_and_other(rng)
    sp.add("v", pa.int64(), list(range(n)), True, "plain")
    return sp.write("delta_ts", out_dir)


def dict_value(typ, j):
    """Entry j of a column's dictionary: distinct for distinct j."""
    if typ == "i64":
        x = (j * 0x9E3779B97F4A7C15 + 12345) & (2**64 - 1)
        return x - 2**64 if x >= 2**63 else x
    if typ == "f64":
        return j * 0.5 - 7.25
    return f"v{j:06d}"


def _dict_indices(d, n, rng):
    """Every entry once in shuffled order (bit-packed), then long repeats of
    lengths that are not all multiples of 8 (RLE) between shuffled stretches."""
    out = [int(x) for x in rng.permutation(d)]
    run_lens = (13, 100, 9, 8, 7, 64, 65, 1, 250, 17)
    mix_lens = (5, 50, 23, 8, 129)
    i = 0
    while len(out) < n:
        out += [int(rng.integers(0, d))] * run_lens[i % len(run_lens)]
        out += [int(x) for x in rng.integers(0, d, mix_lens[i % len(mix_lens)])]
        i += 1
    return out[:n]


_PA_TYPES = {"i64": pa.int64(), "f64": pa.float64(), "str": pa.string()}


def dict_case(out_dir, size_class, variant, compression="lz4", tag=None):
    """x_<type>_<D>: dictionary-encoded columns with D entries. size_class
    'small' (DICT_SIZES_SMALL, 9,000 rows) or 'big' (DICT_SIZES_BIG, 70,000
    rows). variant: req / nn / nul, or 'mp' (nulls, several pages)."""
    sizes, n = ((DICT_SIZES_SMALL, DICT_ROWS_SMALL) if size_class == "small"
                else (DICT_SIZES_BIG, DICT_ROWS_BIG))
    rng = np.random.default_rng(2000 + n)
    sp = _Spec(n)
    sp.add_key_and_other(rng)
    for d in sizes:
        idx = _dict_indices(d, n, rng)
        # big dictionaries: few enough nulls that every entry still occurs
        mask = _null_mask(n, rng, 0.25 if size_class == "small" else 0.04)
        for typ in DICT_TYPES:
            entries = [dict_value(typ, j) for j in range(d)]
            vals = [entries[j] for j in idx]
            if variant in ("nul", "mp"):
                vals = _with_nulls(vals, mask)
            sp.add(f"x_{typ}_{d}", _PA_TYPES[typ], vals, variant != "req",
                   "dict")
    name = tag or f"dict_{size_class}_{variant}"
    return sp.write(name, out_dir, compression, multipage=(variant == "mp"))


def def_mask(layout, n):
    """True = valid."""
    m = np.ones(n, dtype=bool)
    if layout == "all_null":
        m[:] = False
    elif layout == "null_first":
        m[0] = False
    elif layout == "null_last":
        m[n - 1] = False
    elif layout == "alt":
        m[1::2] = False
    elif layout == "runs":
        pos = 0
        for length in DEF_RUN_LENGTHS:     # L valid rows, then L nulls
            m[pos + length:pos + 2 * length] = False
            pos += 2 * length
        m[pos::3] = False                  # tail: mixed
    else:
        assert layout == "all_valid"
    return m


def def_case(out_dir, multipage=False):
    """i_<layout>: nullable INT64 PLAIN; s_<layout>: nullable utf8
    dictionary; one pair per DEF_LAYOUTS."""
    n = DEF_ROWS
    rng = np.random.default_rng(3000)
    sp = _Spec(n)
    sp.add_key_and_other(rng)
    words = [f"w{j:02d}" for j in range(37)]
    for layout in DEF_LAYOUTS:
        m = def_mask(layout, n)
        iv = [int(x) for x in rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64)]
        sv = [words[int(x)] for x in rng.integers(0, len(words), n)]
        sp.add(f"i_{layout}", pa.int64(), _with_nulls(iv, m), True, "plain")
        sp.add(f"s_{layout}", pa.string(), _with_nulls(sv, m), True, "dict")
    return sp.write("def_mp" if multipage else "def", out_dir,
                    multipage=multipage)


def _i32_values(kind, n, rng):
    edge = [I32_MIN, I32_MAX, -1, 0, 1, I32_MIN + 1, I32_MAX - 1]
    if kind == "dict":     # 300 entries, extremes among them
        entries = edge + [int(x) for x in rng.integers(I32_MIN, I32_MAX, 293)]
        return [entries[j] for j in _dict_indices(len(entries), n, rng)]
    v = [int(x) for x in rng.integers(I32_MIN, I32_MAX, n, endpoint=True)]
    if kind == "delta":    # deltas of +-(2**32 - 1): wrap at 32 bits
        for i in range(min(n, 200)):
            v[i] = I32_MIN if i % 2 else I32_MAX
    v[200:200 + len(edge)] = edge
    return v


def int32_case(out_dir):
    """i32_<kind>_<variant> for INT32_KINDS, plus i64_plain_* and f64_plain_*
    (8-byte PLAIN pages, required and nullable)."""
    n = INT32_ROWS
    rng = np.random.default_rng(4000)
    sp = _Spec(n)
    sp.add_key_and_other(rng)
    for kind in INT32_KINDS:
        sp.add_variants(f"i32_{kind}", pa.int32(), _i32_values(kind, n, rng),
                        kind, rng)
    sp.add_variants("i64_plain", pa.int64(), _delta_values(64, n, rng),
                    "plain", rng)
    sp.add_variants("f64_plain", pa.float64(),
                    [float(x) for x in rng.standard_normal(n) * 1e6],
                    "plain", rng)
    return sp.write("int32", out_dir)


def int32_overflow_case(out_dir):
    """i32_ovf_<variant>: dictionary enabled but limited to 1 KiB, so the
    chunk starts with a dictionary-encoded page and falls back to PLAIN."""
    n = INT32_ROWS
    rng = np.random.default_rng(4001)
    sp = _Spec(n)
    sp.add_key_and_other(rng)
    sp.add_variants("i32_ovf", pa.int32(), _i32_values("plain", n, rng),
                    "dict", rng)
    return sp.write("int32_ovf", out_dir, multipage=True, dict_limit=1024)


# ---------------------------------------------------------------------------
# page inspector
# ---------------------------------------------------------------------------

ENCODINGS = {0: "PLAIN", 2: "PLAIN_DICTIONARY", 3: "RLE", 4: "BIT_PACKED",
             5: "DELTA_BINARY_PACKED", 6: "DELTA_LENGTH_BYTE_ARRAY",
             7: "DELTA_BYTE_ARRAY", 8: "RLE_DICTIONARY", 9: "BYTE_STREAM_SPLIT"}
DICT_ENCODINGS = ("PLAIN_DICTIONARY", "RLE_DICTIONARY")


def _uvarint(buf, pos):
    v = shift = 0
    while True:
        b = buf[pos]
        pos += 1
        v |= (b & 0x7F) << shift
        if not b & 0x80:
            return v, pos
        shift += 7


def _unzigzag(v):
    return (v >> 1) ^ -(v & 1)


def _thrift_value(buf, pos, t):
    if t in (1, 2):
        return t == 1, pos
    if t == 3:
        return buf[pos], pos + 1
    if t in (4, 5, 6):
        v, pos = _uvarint(buf, pos)
        return _unzigzag(v), pos
    if t == 7:
        return struct.unpack_from("<d", buf, pos)[0], pos + 8
    if t == 8:
        ln, pos = _uvarint(buf, pos)
        return bytes(buf[pos:pos + ln]), pos + ln
    if t in (9, 10):
        h = buf[pos]
        pos += 1
        size, et = h >> 4, h & 15
        if size == 15:
            size, pos = _uvarint(buf, pos)
        out = []
        for _ in range(size):
            if et in (1, 2):       # list<bool>: one byte per element
                out.append(buf[pos] == 1)
                pos += 1
            else:
                v, pos = _thrift_value(buf, pos, et)
                out.append(v)
        return out, pos
    if t == 12:
        return thrift_struct(buf, pos)
    raise ValueError(f"thrift compact type {t} not handled")


def thrift_struct(buf, pos):
    """Thrift compact struct at buf[pos:] -> ({field id: value}, end pos).
    Nested structs are dicts; maps do not occur in a PageHeader."""
    out, fid = {}, 0
    while True:
        h = buf[pos]
        pos += 1
        if h == 0:
            return out, pos
        delta, t = h >> 4, h & 15
        if delta:
            fid += delta
        else:
            v, pos = _uvarint(buf, pos)
            fid = _unzigzag(v)
        out[fid], pos = _thrift_value(buf, pos, t)


def _wrap(x, bits):
    x &= (1 << bits) - 1
    return x - (1 << bits) if x >> (bits - 1) else x


def decode_hybrid(buf, pos, bw, n):
    """RLE/bit-packed hybrid: n values of bit width bw from buf[pos:] ->
    (values, runs, end pos); runs = [(kind, start, length)], kind 'rle' or
    'packed', start = index of the run's first value, length clipped to n."""
    vals, runs = [], []
    mask = (1 << bw) - 1
    byte_w = (bw + 7) // 8
    while len(vals) < n:
        hdr, pos = _uvarint(buf, pos)
        start = len(vals)
        if hdr & 1:
            groups = hdr >> 1
            for _ in range(groups):
                g = int.from_bytes(buf[pos:pos + bw], "little")
                pos += bw
                for k in range(8):
                    if len(vals) < n:
                        vals.append((g >> (k * bw)) & mask)
            runs.append(("packed", start, len(vals) - start))
        else:
            cnt = hdr >> 1
            v = int.from_bytes(buf[pos:pos + byte_w], "little")
            pos += byte_w
            take = min(cnt, n - len(vals))
            vals.extend([v] * take)
            runs.append(("rle", start, take))
    return vals, runs, pos


def decode_delta(buf, pos, bits=64):
    """DELTA_BINARY_PACKED from buf[pos:], sums wrapping at `bits` (64, or
    32 for INT32) -> (values, info). info: block size, miniblocks per block,
    widths = [(bit width, deltas held)] per miniblock that holds any, and
    each block's min_delta."""
    block, pos = _uvarint(buf, pos)
    mpb, pos = _uvarint(buf, pos)
    total, pos = _uvarint(buf, pos)
    first, pos = _uvarint(buf, pos)
    value = _wrap(_unzigzag(first), bits)
    per_mini = block // mpb
    vals = [value] if total else []
    widths, min_deltas = [], []
    while len(vals) < total:
        md, pos = _uvarint(buf, pos)
        md = _unzigzag(md)
        min_deltas.append(md)
        bws = buf[pos:pos + mpb]
        pos += mpb
        for bw in bws:
            if len(vals) >= total:
                break              # unused miniblock: width byte only
            nbytes = per_mini * bw // 8
            packed = int.from_bytes(buf[pos:pos + nbytes], "little")
            pos += nbytes
            take = min(per_mini, total - len(vals))
            mask = (1 << bw) - 1
            for i in range(take):
                value = _wrap(value + md + ((packed >> (i * bw)) & mask), bits)
                vals.append(value)
            widths.append((bw, take))
    return vals, {"block": block, "miniblocks": mpb, "per_mini": per_mini,
                  "widths": widths, "min_deltas": min_deltas}


def decode_plain(buf, pos, phys, n):
    out = []
    if phys == "BYTE_ARRAY":
        for _ in range(n):
            ln = int.from_bytes(buf[pos:pos + 4], "little")
            out.append(bytes(buf[pos + 4:pos + 4 + ln]).decode())
            pos += 4 + ln
        return out
    w = {"INT32": 4, "INT64": 8, "DOUBLE": 8}[phys]
    for i in range(n):
        chunk = buf[pos + i * w:pos + (i + 1) * w]
        assert len(chunk) == w, "PLAIN page shorter than its value count"
        out.append(struct.unpack("<d", chunk)[0] if phys == "DOUBLE"
                   else int.from_bytes(chunk, "little", signed=True))
    return out


_CODECS = {"SNAPPY": ("snappy",), "LZ4": ("lz4_raw", "lz4_hadoop"),
           "LZ4_RAW": ("lz4_raw",)}


def _decompress(codec, comp, uncomp):
    if codec == "UNCOMPRESSED":
        return bytes(comp)
    err = None
    for name in _CODECS[codec]:
        try:
            return pa.Codec(name).decompress(comp, uncomp).to_pybytes()
        except Exception as e:   # the legacy LZ4 id covers two framings
            err = e
    raise err


def inspect_file(path):
    """{column name: info}. info: phys, optional, values (decoded column,
    None = NULL) and pages, one dict per data page: encoding, num_values,
    def_runs (None for a required column), and for dictionary pages idx_bw
    and idx_runs, for delta pages delta (see decode_delta)."""
    pf = pq.ParquetFile(path)
    md = pf.metadata
    assert md.num_row_groups == 1
    rg = md.row_group(0)
    raw = open(path, "rb").read()
    out = {}
    for ci in range(rg.num_columns):
        cc = rg.column(ci)
        sc = pf.schema.column(ci)
        assert sc.max_repetition_level == 0 and sc.max_definition_level <= 1
        optional = sc.max_definition_level == 1
        phys = cc.physical_type
        pos = cc.data_page_offset
        if cc.has_dictionary_page and cc.dictionary_page_offset:
            pos = min(pos, cc.dictionary_page_offset)
        dictionary, values, pages = None, [], []
        while len(values) < cc.num_values:
            ph, pos = thrift_struct(raw, pos)
            body = _decompress(cc.compression, raw[pos:pos + ph[3]], ph[2])
            pos += ph[3]
            if ph[1] == 2:                       # DICTIONARY_PAGE
                dictionary = decode_plain(body, 0, phys, ph[7][1])
                continue
            assert ph[1] == 0, "only data page v1 is written here"
            dh = ph[5]
            nv, enc = dh[1], ENCODINGS[dh[2]]
            page = {"encoding": enc, "num_values": nv, "def_runs": None}
            p = 0
            defs = [1] * nv
            if optional:
                assert ENCODINGS[dh[3]] == "RLE"
                dl = int.from_bytes(body[0:4], "little")
                defs, page["def_runs"], end = decode_hybrid(body, 4, 1, nv)
                assert end <= 4 + dl
                p = 4 + dl
            present = sum(defs)
            if enc in DICT_ENCODINGS:
                bw = body[p]
                page["idx_bw"] = bw
                if bw == 0 and p + 1 >= len(body):
                    idx, page["idx_runs"] = [0] * present, []
                else:
                    idx, page["idx_runs"], _ = decode_hybrid(body, p + 1, bw,
                                                             present)
                dense = [dictionary[j] for j in idx]
            elif enc == "DELTA_BINARY_PACKED":
                dense, page["delta"] = decode_delta(
                    body, p, 32 if phys == "INT32" else 64)
                assert len(dense) == present
            else:
                assert enc == "PLAIN", enc
                dense = decode_plain(body, p, phys, present)
            it = iter(dense)
            values.extend(next(it) if d else None for d in defs)
            pages.append(page)
        out[sc.path] = {"phys": phys, "optional": optional, "values": values,
                        "pages": pages, "codec": cc.compression}
    return out


def same_value(a, b):
    """Exact equality; doubles by bit pattern."""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, float) or isinstance(b, float):
        return struct.pack("<d", a) == struct.pack("<d", b)
    return a == b


def first_mismatch(got, want):
    """None when the sequences are equal element by element, else a short
    description of the first difference."""
    if len(got) != len(want):
        return f"length {len(got)} != {len(want)}"
    for i, (g, w) in enumerate(zip(got, want)):
        if not same_value(g, w):
            return f"row {i}: got {g!r}, want {w!r}"
    return None


# ---------------------------------------------------------------------------
# query reference over the source arrays
# ---------------------------------------------------------------------------

def _pred_ok(p, v):
    op = p["op"]
    if op == "is_null":
        return v is None
    if op == "is_not_null":
        return v is not None
    if v is None:
        return False              # a comparison never matches NULL
    lit = p["lit"]
    return {"eq": v == lit, "ne": v != lit, "lt": v < lit, "le": v <= lit,
            "gt": v > lit, "ge": v >= lit}[op]


def ref_query(case, q):
    """The query over case.cols in plain Python (exact ints): rows in the
    engine's normalized form. Projections: rows in p_timestamp DESC order.
    Aggregations: [key, aggs...] sorted by key, the NULL key last; count
    aggregates are 0 and the others None over no values."""
    n = case.n
    sel = [i for i in range(n)
           if all(_pred_ok(p, case.cols[p["col"]][i])
                  for p in q.get("preds", []))]
    if q.get("select_cols"):
        ts = case.cols["p_timestamp"]
        sel.sort(key=lambda i: -ts[i])
        if q.get("limit"):
            sel = sel[:q["limit"]]
        return [[case.cols[c][i] for c in q["select_cols"]] for i in sel]
    gb = q.get("group_by", [])
    assert len(gb) <= 1
    groups = {}
    for i in sel:
        groups.setdefault(case.cols[gb[0]][i] if gb else (), []).append(i)
    if not gb and not groups:
        groups[()] = []
    rows = []
    for key in sorted(groups, key=lambda k: (k is None, 0 if k is None else k)):
        row = [key] if gb else []
        for a in q["select"]:
            if a["agg"] == "count_star":
                row.append(len(groups[key]))
                continue
            vals = [case.cols[a["col"]][i] for i in groups[key]]
            vals = [v for v in vals if v is not None]
            if a["agg"] == "count":
                row.append(len(vals))
            elif a["agg"] == "count_distinct":
                row.append(len(set(vals)))
            elif not vals:
                row.append(None)
            else:
                row.append({"min": min, "max": max, "sum": sum}[a["agg"]](vals))
        rows.append(row)
    return rows


# ---------------------------------------------------------------------------
# the case set shared by the CPU and GPU test modules
# ---------------------------------------------------------------------------

CODEC_TWINS = ("snappy", "none")


def _builders():
    b = {}
    for n in DELTA_ROWS:
        b[f"delta_{n}"] = lambda d, n=n: delta_case(d, n)
    b[f"delta_mp_{DELTA_MP_ROWS}"] = lambda d: delta_case(
        d, DELTA_MP_ROWS, multipage=True)
    b["delta_ts"] = delta_ts_case
    for sc in ("small", "big"):
        for v in VARIANTS + ("mp",):
            b[f"dict_{sc}_{v}"] = lambda d, sc=sc, v=v: dict_case(d, sc, v)
    b["def"] = def_case
    b["def_mp"] = lambda d: def_case(d, multipage=True)
    b["int32"] = int32_case
    b["int32_ovf"] = int32_overflow_case
    for codec in CODEC_TWINS:    # decode failures must not pass for codec ones
        b[f"delta_1000_{codec}"] = lambda d, c=codec: delta_case(
            d, 1000, c, tag=f"delta_1000_{c}")
        b[f"dict_small_nul_{codec}"] = lambda d, c=codec: dict_case(
            d, "small", "nul", c, tag=f"dict_small_nul_{c}")
    return b


BUILDERS = _builders()
CASE_NAMES = tuple(BUILDERS)


class CaseSet:
    """Cases written on first use into one directory, and their inspections."""

    def __init__(self, out_dir):
        self.out_dir = str(out_dir)
        self._cases, self._info = {}, {}

    def case(self, name):
        if name not in self._cases:
            self._cases[name] = BUILDERS[name](self.out_dir)
        return self._cases[name]

    def info(self, name):
        if name not in self._info:
            self._info[name] = inspect_file(self.case(name).path)
        return self._info[name]


# ---------------------------------------------------------------------------
# files the engine must refuse at plan build (not decoded by the inspector)
# ---------------------------------------------------------------------------

def unsupported_types_case(out_dir, n=500):
    """b BOOLEAN, f FLOAT, x FIXED_LEN_BYTE_ARRAY(4), all PLAIN."""
    rng = np.random.default_rng(5000)
    path = os.path.join(out_dir, "unsupported_types.parquet")
    tbl = pa.table({
        "p_timestamp": pa.array([TS0 + 7 * (n - 1 - i) for i in range(n)],
                                type=pa.timestamp("ms")),
        "b": pa.array([bool(x) for x in rng.integers(0, 2, n)]),
        "f": pa.array(rng.standard_normal(n), type=pa.float32()),
        "x": pa.array([int(v).to_bytes(4, "little") for v in
                       rng.integers(0, 2**32, n)], type=pa.binary(4)),
    })
    pq.write_table(tbl, path, compression="lz4", use_dictionary=False,
                   data_page_version="1.0")
    return path


def int96_case(out_dir, n=500):
    """t96: a nanosecond timestamp written as INT96."""
    path = os.path.join(out_dir, "int96.parquet")
    tbl = pa.table({
        "p_timestamp": pa.array([TS0 + 7 * (n - 1 - i) for i in range(n)],
                                type=pa.int64()),
        "t96": pa.array([TS0 * 10**6 + i for i in range(n)],
                        type=pa.timestamp("ns")),
    })
    pq.write_table(tbl, path, compression="lz4", use_dictionary=False,
                   data_page_version="1.0",
                   use_deprecated_int96_timestamps=True)
    return path


def page_v2_case(out_dir, n=500):
    """v: INT64 PLAIN in data page v2."""
    path = os.path.join(out_dir, "page_v2.parquet")
    tbl = pa.table({
        "p_timestamp": pa.array([TS0 + 7 * (n - 1 - i) for i in range(n)],
                                type=pa.timestamp("ms")),
        "v": pa.array(list(range(n)), type=pa.int64()),
    })
    pq.write_table(tbl, path, compression="lz4", use_dictionary=False,
                   data_page_version="2.0")
    return path


def first_page_types(path):
    """{column: (physical type, PageHeader.type of the chunk's first page)}"""
    pf = pq.ParquetFile(path)
    rg = pf.metadata.row_group(0)
    raw = open(path, "rb").read()
    out = {}
    for ci in range(rg.num_columns):
        cc = rg.column(ci)
        pos = cc.data_page_offset
        if cc.has_dictionary_page and cc.dictionary_page_offset:
            pos = min(pos, cc.dictionary_page_offset)
        ph, _ = thrift_struct(raw, pos)
        out[cc.path_in_schema] = (cc.physical_type, ph[1])
    return out
