"""The page-case fixtures (tests/pagecases_common.py) checked without the
code under test: the page inspector's decode of every column equals the
source arrays the file was written from, and every file contains the page
shapes it is there for. The second part is what keeps tests/
test_gpu_pagecases.py honest: if a pyarrow upgrade changes what the writer
emits (another delta block size, no RLE runs, another page split), a
condition here fails instead of the GPU test silently losing its coverage.

Shapes pyarrow's writer does not produce, so no fixture has them:
  - dictionary index bit width 0: a one-entry dictionary is written with
    width 1; width 0 appears only on pages that hold no value at all
    (s_all_null), where there is no index run to decode;
  - a null-free page whose def levels are two separate RLE runs: the level
    encoder merges adjacent equal runs within a page.
"""

import collections

import pytest

from tests import pagecases_common as pc


@pytest.fixture(scope="module")
def cs(tmp_path_factory):
    return pc.CaseSet(tmp_path_factory.mktemp("pagecases_cpu"))


def _delta_widths(col_info):
    return [w for p in col_info["pages"] for w in p["delta"]["widths"]]


def _run_kinds(pages, key):
    return collections.Counter(r[0] for p in pages for r in (p[key] or ()))


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_inspector_decode_equals_source(cs, name):
    """Validates inspector and fixtures against each other: arbitrary-
    precision decode of every page == the arrays handed to the writer."""
    case, info = cs.case(name), cs.info(name)
    assert set(info) == set(case.cols)
    for col, src in case.cols.items():
        bad = pc.first_mismatch(info[col]["values"], list(src))
        assert bad is None, f"{name}.{col}: {bad}"


@pytest.mark.parametrize("name", pc.CASE_NAMES)
def test_variants_have_their_def_level_shape(cs, name):
    """_req: no def levels; _nn: one RLE run of ones per page; _nul: nulls,
    with both run kinds in the def levels of files large enough."""
    case, info = cs.case(name), cs.info(name)
    for col in case.cols:
        ci = info[col]
        if col.endswith("_req") or name.endswith("_req") and col.startswith("x_"):
            assert not ci["optional"], col
            assert all(p["def_runs"] is None for p in ci["pages"]), col
        elif col.endswith("_nn") or name.endswith("_nn") and col.startswith("x_"):
            assert ci["optional"], col
            for p in ci["pages"]:
                assert p["def_runs"] == [("rle", 0, p["num_values"])], col
        elif col.endswith("_nul") or (
                name.rsplit("_", 1)[-1] in ("nul", "mp") + pc.CODEC_TWINS
                and col.startswith("x_")):
            assert ci["optional"], col
            assert any(v is None for v in case.cols[col]) or case.n < 2, col
            if case.n >= 256:
                assert set(_run_kinds(ci["pages"], "def_runs")) == {
                    "rle", "packed"}, col


@pytest.mark.parametrize("name", [f"delta_{n}" for n in (256, 257, 1000)]
                         + [f"delta_mp_{pc.DELTA_MP_ROWS}"]
                         + [f"delta_1000_{c}" for c in pc.CODEC_TWINS])
def test_delta_widths_present(cs, name):
    info = cs.info(name)
    for v in pc.VARIANTS:
        for b in pc.DELTA_WIDTHS:
            ci = info[f"d_{b}_{v}"]
            assert ci["phys"] == "INT64"
            assert all(p["encoding"] == "DELTA_BINARY_PACKED"
                       for p in ci["pages"])
            widths = _delta_widths(ci)
            assert b in {w for w, _ in widths}, (name, b, v, widths)
            assert max(w for w, _ in widths) <= b
            if b in pc.DELTA_HARD_WIDTHS:
                per_mini = ci["pages"][0]["delta"]["per_mini"]
                assert (b, per_mini) in widths, (
                    f"{name} d_{b}_{v}: no full miniblock of width {b}")
        assert {w for w, _ in _delta_widths(info[f"d_const_{v}"])} == {0}
        dec = info[f"d_dec_{v}"]["pages"]
        assert all(md < 0 for p in dec for md in p["delta"]["min_deltas"])
        alt = [x for x in cs.case(name).cols[f"d_alt_{v}"] if x is not None]
        assert {pc.I64_MIN, pc.I64_MAX} == set(alt)   # deltas wrap at 64 bits


def test_delta_row_counts_hit_the_block_edges(cs):
    """1 row: first value only; 2: one delta; 65: exactly one miniblock;
    257: exactly one block; 1000: a partial last miniblock."""
    def shape(n):
        d = cs.info(f"delta_{n}")["d_59_req"]["pages"][0]["delta"]
        return d, [c for _, c in d["widths"]]

    d, counts = shape(1)
    # DELTA_ROWS is chosen for 64-value miniblocks in blocks of 256: another
    # writer layout needs another list
    assert (d["per_mini"], d["block"], d["miniblocks"]) == (64, 256, 4)
    assert counts == []
    assert shape(2)[1] == [1]
    assert shape(64)[1] == [63]
    assert shape(65)[1] == [64]
    assert shape(256)[1] == [64, 64, 64, 63]
    assert shape(257)[1] == [64, 64, 64, 64]
    assert shape(1000)[1][-1] == 999 % 64


@pytest.mark.parametrize("name", [f"delta_mp_{pc.DELTA_MP_ROWS}",
                                  "dict_small_mp", "dict_big_mp", "def_mp",
                                  "int32_ovf"])
def test_multipage_files(cs, name):
    info = cs.info(name)
    for col, ci in info.items():
        if all(v is None for v in ci["values"]):
            continue   # no value bytes: the writer never sees a full page
        rows = [p["num_values"] for p in ci["pages"]]
        assert len(rows) >= 3, (name, col, rows)
        assert any(r % 64 for r in rows[:-1]), (name, col, rows)
        assert any(r % 8 for r in rows), (name, col, rows)


def test_delta_timestamp_is_out_of_order_by_hours(cs):
    case, info = cs.case("delta_ts"), cs.info("delta_ts")
    assert {p["encoding"] for p in info["p_timestamp"]["pages"]} == {
        "DELTA_BINARY_PACKED"}
    ts = list(case.cols["p_timestamp"])
    assert len(set(ts)) == len(ts)
    d = [b - a for a, b in zip(ts, ts[1:])]
    hour = 3_600_000
    assert sum(x > hour for x in d) > 100 and sum(x < -hour for x in d) > 100


def test_dict_index_widths_and_run_kinds(cs):
    """Every reachable width in DICT_INDEX_WIDTHS occurs for each value type
    on a page with both an RLE and a bit-packed run; RLE run lengths include
    non-multiples of 8; no page fell back to PLAIN."""
    both = collections.defaultdict(set)     # type -> widths with both kinds
    odd_rle = False
    for name in pc.CASE_NAMES:
        if not name.startswith("dict_"):
            continue
        for col, ci in cs.info(name).items():
            if not col.startswith("x_"):
                continue
            typ = col.split("_")[1]
            for p in ci["pages"]:
                assert p["encoding"] in pc.DICT_ENCODINGS, (name, col)
                kinds = {r[0] for r in p["idx_runs"]}
                if kinds == {"rle", "packed"}:
                    both[typ].add(p["idx_bw"])
                odd_rle |= any(k == "rle" and ln % 8 for k, _, ln
                               in p["idx_runs"])
    want = set(pc.DICT_INDEX_WIDTHS) - {0}
    for typ in pc.DICT_TYPES:
        assert want <= both[typ], (typ, sorted(want - both[typ]))
    assert odd_rle


def test_dict_sizes_are_what_the_names_say(cs):
    for name in ("dict_small_req", "dict_small_nul", "dict_big_nn",
                 "dict_big_mp"):
        case = cs.case(name)
        for col, src in case.cols.items():
            if col.startswith("x_"):
                d = int(col.split("_")[2])
                assert len({v for v in src if v is not None}) == d, (name, col)


def test_def_patterns(cs):
    info = cs.info("def")
    case = cs.case("def")
    assert case.n % 8
    for pre in ("i_", "s_"):
        runs = info[pre + "runs"]["pages"][0]["def_runs"]
        assert any(k == "packed" and s % 8 for k, s, _ in runs), runs
        assert any(k == "rle" and s // 64 != (s + ln - 1) // 64
                   for k, s, ln in runs), runs
        rle_lens = {ln for k, _, ln in runs if k == "rle"}
        assert {9, 63, 64, 65, 1000} <= rle_lens, rle_lens
        assert info[pre + "all_null"]["pages"][0]["def_runs"] == [
            ("rle", 0, case.n)]
        assert info[pre + "all_valid"]["pages"][0]["def_runs"] == [
            ("rle", 0, case.n)]
        assert all(v is None for v in case.cols[pre + "all_null"])
        assert case.cols[pre + "null_first"][0] is None
        assert case.cols[pre + "null_last"][-1] is None
        assert _run_kinds(info[pre + "alt"]["pages"], "def_runs")["packed"]
    for layout in pc.DEF_LAYOUTS:
        assert {p["encoding"] for p in info[f"i_{layout}"]["pages"]} == {"PLAIN"}
        assert {p["encoding"] for p in info[f"s_{layout}"]["pages"]} <= set(
            pc.DICT_ENCODINGS)
    # the only place index width 0 occurs: pages without a single value
    assert info["s_all_null"]["pages"][0]["idx_bw"] == 0
    # several pages: runs begin mid-page at other offsets
    mp = cs.info("def_mp")["i_runs"]["pages"]
    assert any(k == "packed" and s % 8 for p in mp for k, s, _ in p["def_runs"])


def test_int32_pages(cs):
    info, ovf = cs.info("int32"), cs.info("int32_ovf")
    want = {"dict": set(pc.DICT_ENCODINGS), "plain": {"PLAIN"},
            "delta": {"DELTA_BINARY_PACKED"}}
    for kind in pc.INT32_KINDS:
        for v in pc.VARIANTS:
            ci = info[f"i32_{kind}_{v}"]
            assert ci["phys"] == "INT32"
            assert {p["encoding"] for p in ci["pages"]} <= want[kind]
            src = [x for x in cs.case("int32").cols[f"i32_{kind}_{v}"]
                   if x is not None]
            assert {pc.I32_MIN, pc.I32_MAX, -1} <= set(src)
    for v in pc.VARIANTS:
        src = [x for x in cs.case("int32").cols[f"i32_delta_{v}"]
               if x is not None]
        assert abs(src[1] - src[0]) >= 2**31        # the delta wraps
        ci = ovf[f"i32_ovf_{v}"]
        assert ci["phys"] == "INT32"
        encs = [p["encoding"] for p in ci["pages"]]
        assert encs[0] in pc.DICT_ENCODINGS and "PLAIN" in encs, encs
        assert info[f"i64_plain_{v}"]["phys"] == "INT64"
        assert info[f"f64_plain_{v}"]["phys"] == "DOUBLE"
        for stem in ("i64_plain", "f64_plain"):
            assert {p["encoding"] for p in info[f"{stem}_{v}"]["pages"]} == {
                "PLAIN"}


def test_codec_twins(cs):
    for base, twins in (("delta_1000", "delta_1000_"),
                        ("dict_small_nul", "dict_small_nul_")):
        assert {ci["codec"] for ci in cs.info(base).values()} <= {
            "LZ4", "LZ4_RAW"}
        assert {ci["codec"] for ci in cs.info(twins + "snappy").values()} == {
            "SNAPPY"}
        assert {ci["codec"] for ci in cs.info(twins + "none").values()} == {
            "UNCOMPRESSED"}
        for codec in pc.CODEC_TWINS:   # same data, whatever the codec
            a, b = cs.case(base), cs.case(twins + codec)
            assert all(pc.first_mismatch(list(a.cols[c]), list(b.cols[c]))
                       is None for c in a.cols)


QUERIES = [
    ("int32", {"select": [{"agg": "count_star"},
                          {"agg": "max", "col": "i32_plain_req"}],
               "group_by": ["k"]}),
    ("int32", {"select": [{"agg": "count_star"}], "group_by": ["i32_dict_nul"]}),
    ("delta_1000", {"select": [{"agg": "count_star"},
                               {"agg": "min", "col": "d_63_nn"}],
                    "group_by": ["k"],
                    "preds": [{"col": "d_33_req", "op": "ge", "lit": 2**31}]}),
    ("dict_small_nul", {"select": [{"agg": "count_star"},
                                   {"agg": "count", "col": "x_str_257"}],
                        "preds": [{"col": "x_i64_9", "op": "ne",
                                   "lit": pc.dict_value("i64", 3)}]}),
    ("def", {"select_cols": ["p_timestamp", "s_runs", "i_alt"], "limit": 2507}),
]


@pytest.mark.parametrize("i", range(len(QUERIES)))
def test_reference_agrees_with_the_oracle(cs, i):
    """ref_query (exact Python over the source arrays) is the GPU tests'
    reference; here it is pinned against the pyarrow/numpy oracle on queries
    the oracle evaluates exactly."""
    from oracle import query_oracle as qo
    from oracle.compare import assert_rows_equal

    name, q = QUERIES[i]
    case = cs.case(name)
    want = qo.execute([case.path], dict(q))["rows"]
    assert_rows_equal(pc.ref_query(case, q), want, f"{name}: {q}")


def test_hash_plain_length_wrap_is_refused(tmp_path, monkeypatch):
    """A PLAIN byte-array page of a hash-mode column whose length field
    would wrap 32-bit position arithmetic (pos + 4 + 0xFFFFFFFC == pos mod
    2**32) must fail plan build instead of passing the overrun check and
    handing bogus strrefs to the device. Plan building is pure host work
    (GPUQ_FAKE_DEVICE)."""
    import pyarrow as pa
    import pyarrow.parquet as pq

    from parseable_amd import GpuExecutionPlan, GpuqError, GpuSession

    path = str(tmp_path / "wrap.parquet")
    vals = ["aa", "bbb", "c"]
    tbl = pa.table({
        "p_timestamp": pa.array([pc.TS0 + i for i in range(3)],
                                type=pa.timestamp("ms")),
        "s": pa.array(vals, type=pa.string()),
    })
    pq.write_table(tbl, path, compression="none", use_dictionary=False,
                   data_page_version="1.0", row_group_size=1 << 20)
    # precondition: one v1 PLAIN data page, no dictionary — a dictionary-
    # encoded page would let the plan build pass for nothing
    assert pc.first_page_types(path)["s"] == ("BYTE_ARRAY", 0)
    info = pc.inspect_file(path)["s"]
    assert info["codec"] == "UNCOMPRESSED"
    assert [p["encoding"] for p in info["pages"]] == ["PLAIN"]
    assert info["values"] == vals

    # the page's value block: after the page header and the def levels
    rg = pq.ParquetFile(path).metadata.row_group(0)
    cc = next(rg.column(i) for i in range(rg.num_columns)
              if rg.column(i).path_in_schema == "s")
    raw = bytearray(open(path, "rb").read())
    ph, body = pc.thrift_struct(raw, cc.data_page_offset)
    assert ph[2] == ph[3]                      # stored uncompressed
    p = body
    if info["optional"]:
        p += 4 + int.from_bytes(raw[body:body + 4], "little")
    assert raw[p:p + 6] == (2).to_bytes(4, "little") + b"aa"
    second = p + 4 + len(vals[0])
    assert raw[second:second + 4] == (3).to_bytes(4, "little")
    raw[second:second + 4] = (0xFFFFFFFC).to_bytes(4, "little")
    with open(path, "wb") as fh:
        fh.write(raw)

    monkeypatch.setenv("GPUQ_FAKE_DEVICE", "1")
    q = {"select": [{"agg": "count_star"}], "group_by": ["s"]}
    with pytest.raises(GpuqError, match="plain page overrun"):
        GpuExecutionPlan(GpuSession(), [path], q).close()


def test_refused_files_are_what_they_claim(tmp_path):
    """The files tests/test_gpu_pagecases.py expects plan build to refuse
    really hold BOOLEAN / FLOAT / FLBA / INT96 columns and a v2 data page."""
    t = pc.first_page_types(pc.unsupported_types_case(str(tmp_path)))
    assert (t["b"][0], t["f"][0], t["x"][0]) == (
        "BOOLEAN", "FLOAT", "FIXED_LEN_BYTE_ARRAY")
    assert pc.first_page_types(pc.int96_case(str(tmp_path)))["t96"][0] == "INT96"
    v2 = pc.first_page_types(pc.page_v2_case(str(tmp_path)))
    assert v2["v"] == ("INT64", 3)       # PageType DATA_PAGE_V2
    assert t["b"][1] == 0                # DATA_PAGE (v1) everywhere else
