"""Fixtures for the dictionary run-header scan (dict_page_decode): index
streams whose RLE/bit-packed run structure sits on the edges of the scan,
written with the writers of tests/pagecases_common.py and read back with
its Thrift / hybrid decoders.

The writer closes a bit-packed run at 63 groups (RUN = 504 values, header
byte 0x7F) and starts an RLE run where 8 equal values fill one group, so a
shape is a list of stretches: `packed(n)` values with no two neighbours
equal, and `[RVAL] * c` for an RLE run of c. tests/test_dictwalk_cpu.py
proves with `idx_pages` that each file holds the runs it is named for;
tests/test_gpu_dictwalk.py runs them through every consumer of the decoder.

A fixture is two files of one row group each: `<name>` (columns null-free)
and `<name>_nul` (s and x carry NULLs; the dense stream keeps the shape).
Columns: p_timestamp (unique over all files), k (small utf8 key, distinct
per file), o (INT64 PLAIN), s (utf8 dictionary, the shape) and x (INT64
dictionary, the same shape).
"""

from __future__ import annotations

import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

from tests import pagecases_common as pc

GROUPS = 63                 # groups per full bit-packed run
RUN = GROUPS * 8            # 504 values
RVAL = 0                    # the repeated index of every RLE run
STEP = 64                   # runs one scan step probes

PURE_N = ((1, 7, 8, 9, RUN - 1, RUN, RUN + 1)
          + tuple(k * RUN + e for k in (STEP - 1, STEP, STEP + 1)
                  for e in (-1, 0, 1))
          + (1234,))        # not a multiple of 8: the last run is clipped
RLE_POS = (0, 1, 62, 63, 64, 65, "last")
RLE_COUNTS = (8, 63, 64, 127, 16384)   # 1-, 1-, 2-, 2- and 3-byte headers
WIDTHS = {1: 2, 6: 64, 8: 256, 17: 65537}   # index width -> dictionary size
BIG_WIDTH, BIG_DICT = 20, (1 << 19) + 1     # its own plan: 524,289 entries
MP_PAGES = 5


def packed(n, d, rng, lo=1):
    """n indices from [lo, d) with no two neighbours equal: never an RLE
    run, and never RVAL when lo > RVAL."""
    if d - lo < 2:
        lo = 0
    if d < 2:
        return [0] * n
    v = rng.integers(lo, d, n)
    for i in range(1, n):
        if v[i] == v[i - 1]:
            v[i] = lo + (v[i] - lo + 1) % (d - lo)
    return [int(x) for x in v]


def _decoy(rng):
    """bw = 8 with data bytes equal to the full-run header 0x7F: identity
    first (so that index == value), an RLE run, three full runs, another RLE
    run (the mismatch), then runs of indices 126/127 the stale probes land in."""
    def pair(n):
        v = rng.integers(126, 128, n)
        for i in range(6, n):
            if (v[i - 6:i] == v[i]).all():
                v[i] = 253 - v[i]
        return [int(x) for x in v]
    return (list(range(256)) + [5] * 8 + pair(3 * RUN) + [5] * 8
            + pair(12 * RUN + 3))


def shapes():
    """{name: dense index list}; every list is deterministic."""
    rng = np.random.default_rng(777)
    out = {}
    for n in PURE_N:
        out[f"pure_{n}"] = packed(n, 64, rng, 0)
    for pos in RLE_POS:
        for c in RLE_COUNTS:
            before = (STEP + 2 if pos == "last" else pos) * RUN
            after = 0 if pos == "last" else 2 * RUN + 5
            out[f"rle_{pos}_{c}"] = (packed(before, 64, rng) + [RVAL] * c
                                     + packed(after, 64, rng))
    out["cut"] = packed(80, 64, rng) + [RVAL] * 20 + packed(5 * RUN + 3, 64, rng)
    alt = []
    for _ in range(200):
        alt += packed(16, 64, rng) + [RVAL] * 9
    out["alt"] = alt
    out["decoy"] = _decoy(rng)
    for bw, d in WIDTHS.items():
        n = max((STEP + 3) * RUN + 1, d + 2 * RUN)
        out[f"bw{bw}"] = list(range(d)) + packed(n - d, d, rng, 0)
    out["one"] = [0] * 100          # a one-entry dictionary
    out["mp"] = packed(MP_PAGES * pc.MP_BATCH, 64, rng, 0)
    return out


def big_shape():
    rng = np.random.default_rng(778)
    return list(range(BIG_DICT)) + packed(2 * RUN + 1, BIG_DICT, rng, 0)


def null_rows(n):
    """Validity of the _nul twin: n valid rows, every fourth row NULL, a
    long valid stretch first (so that multi-page files have all-valid pages)
    and a NULL last."""
    m, valid = [], 0
    while valid < n:
        m.append(len(m) < 2 * pc.MP_BATCH or len(m) % 4 != 3)
        valid += m[-1]
    return m + [False]


def write_fixture(out_dir, name, idx, file_no, nul, with_s=True):
    """One file of the fixture -> pc.Case."""
    mask = null_rows(len(idx)) if nul else [True] * len(idx)
    rows = len(mask)
    rng = np.random.default_rng(9000 + file_no)
    sp = pc._Spec(rows, [pc.TS0 + 10_000_000 * file_no + 7 * (rows - 1 - i)
                         for i in range(rows)])
    sp.add("k", pa.string(),
           [f"f{file_no:03d}_{int(j)}" for j in rng.integers(0, 5, rows)],
           True, "dict")
    sp.add("o", pa.int64(), [int(x) for x in rng.integers(-10**6, 10**6, rows)],
           True, "plain")
    s = [f"v{j:07d}" if with_s else f"v{j % 7}" for j in idx]
    x = [3 * j - 1000 for j in idx]
    sp.add("s", pa.string(), pc._with_nulls(s, mask), True, "dict")
    sp.add("x", pa.int64(), pc._with_nulls(x, mask), True, "dict")
    return _write(sp, name + ("_nul" if nul else ""), out_dir, name == "mp")


def _write(sp, name, out_dir, multipage):
    """pc._Spec.write with the writer's rows-per-page limit lifted: a page
    here has to hold far more than 20,000 values (one page per file, except
    the multi-page fixture: a page per batch of MP_BATCH rows)."""
    path = os.path.join(out_dir, f"{name}.parquet")
    tbl = pa.Table.from_arrays(sp.arrays, schema=pa.schema(sp.fields))
    kw = dict(data_page_size=1 << 30, max_rows_per_page=1 << 30)
    if multipage:
        kw = dict(data_page_size=16, write_batch_size=pc.MP_BATCH)
    pq.write_table(tbl, path, row_group_size=1 << 22, compression="lz4",
                   use_dictionary=list(sp.dict_cols),
                   column_encoding=dict(sp.enc), data_page_version="1.0",
                   write_statistics=True,
                   dictionary_pagesize_limit=256 << 20, **kw)
    return pc.Case(name, path, sp.n, sp.src)


class FixtureSet:
    """All fixtures of one variant written once into a directory, and the
    merged Case (rows of all files) the references are computed over."""

    def __init__(self, out_dir):
        self.out_dir = str(out_dir)
        self.shapes = shapes()
        self._sets = {}

    def cases(self, nul):
        if nul not in self._sets:
            self._sets[nul] = [
                write_fixture(self.out_dir, name, idx, 2 * i + int(nul), nul)
                for i, (name, idx) in enumerate(self.shapes.items())]
        return self._sets[nul]

    def big(self):
        if "big" not in self._sets:
            self._sets["big"] = [write_fixture(
                self.out_dir, f"bw{BIG_WIDTH}", big_shape(), 900, False,
                with_s=False)]
        return self._sets["big"]


def merged(cases):
    """One Case over the rows of all files, in file order."""
    cols = {c: np.concatenate([cs.cols[c] for cs in cases])
            for c in cases[0].cols}
    return pc.Case("merged", "", sum(cs.n for cs in cases), cols)


# ---------------------------------------------------------------------------
# inspector: the index pages of one column
# ---------------------------------------------------------------------------

def idx_pages(path, col):
    """The dictionary-encoded data pages of `col`: one dict per page with
    bw, n (values present), runs [(kind, start, length)], idx (the decoded
    indices) and stream (the bytes of the index stream after the width
    byte). Own page walk over pc's Thrift reader and hybrid decoder; pyarrow
    only decompresses."""
    pf = pq.ParquetFile(path)
    rg = pf.metadata.row_group(0)
    raw = open(path, "rb").read()
    for ci in range(rg.num_columns):
        cc = rg.column(ci)
        if cc.path_in_schema == col:
            break
    else:
        raise KeyError(col)
    optional = pf.schema.column(ci).max_definition_level == 1
    pos = cc.data_page_offset
    if cc.has_dictionary_page and cc.dictionary_page_offset:
        pos = min(pos, cc.dictionary_page_offset)
    pages, seen = [], 0
    while seen < cc.num_values:
        ph, pos = pc.thrift_struct(raw, pos)
        body = pc._decompress(cc.compression, raw[pos:pos + ph[3]], ph[2])
        pos += ph[3]
        if ph[1] == 2:
            continue
        dh = ph[5]
        nv = dh[1]
        seen += nv
        assert pc.ENCODINGS[dh[2]] in pc.DICT_ENCODINGS
        p, present = 0, nv
        if optional:
            dl = int.from_bytes(body[0:4], "little")
            defs, _, _ = pc.decode_hybrid(body, 4, 1, nv)
            present = sum(defs)
            p = 4 + dl
        bw = body[p]
        if bw == 0 and p + 1 >= len(body):
            idx, runs, end = [0] * present, [], p + 1
        else:
            idx, runs, end = pc.decode_hybrid(body, p + 1, bw, present)
        pages.append({"bw": bw, "n": present, "runs": runs, "idx": idx,
                      "stream": bytes(body[p + 1:end])})
    return pages


def headers(page):
    """[(offset in page['stream'], header value, header bytes)] per run."""
    out, pos, buf, bw = [], 0, page["stream"], page["bw"]
    left = page["n"]
    while left > 0:
        hdr, nxt = pc._uvarint(buf, pos)
        out.append((pos, hdr, nxt - pos))
        if hdr & 1:
            pos = nxt + (hdr >> 1) * bw
            left -= min(left, (hdr >> 1) * 8)
        else:
            pos = nxt + (bw + 7) // 8
            left -= min(left, hdr >> 1)
    return out
