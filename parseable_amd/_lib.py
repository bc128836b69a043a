"""ctypes bindings for libgpuq.so (the C-ABI of include/gpuq.h).

The library is the product's compute path: if it cannot be loaded or no GPU
is visible, callers MUST fail — there is no CPU fallback anywhere in
parseable_amd (the oracle is test infrastructure only)."""

from __future__ import annotations

import ctypes as C
import os

_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_DIR, "libgpuq.so")


class GpuqFile(C.Structure):
    _fields_ = [
        ("path", C.c_char_p),
        ("row_groups", C.POINTER(C.c_int32)),
        ("n_row_groups", C.c_int32),
    ]


class GpuqPred(C.Structure):
    _fields_ = [
        ("column", C.c_char_p),
        ("op", C.c_int32),
        ("lit_kind", C.c_int32),
        ("i64", C.c_int64 * 2),
        ("f64", C.c_double * 2),
        ("str", C.c_char_p),
        ("hi_exclusive", C.c_int32),
    ]


class GpuqWhereNode(C.Structure):
    """One node of the WHERE tree over the preds (gpuq_where_node)."""
    _fields_ = [("kind", C.c_int32), ("parent", C.c_int32), ("pred", C.c_int32)]


class GpuqAgg(C.Structure):
    _fields_ = [("op", C.c_int32), ("column", C.c_char_p)]


class GpuqAggFilter(C.Structure):
    """One aggregate's FILTER (WHERE ...) tree (gpuq_agg_filter)."""
    _fields_ = [("agg", C.c_int32), ("nodes", C.POINTER(GpuqWhereNode)),
                ("n_nodes", C.c_int32)]


class GpuqMetrics(C.Structure):
    _fields_ = [
        ("rows_scanned", C.c_int64),
        ("rows_out", C.c_int64),
        ("bytes_scanned", C.c_int64),
        ("rowgroup_bytes_total", C.c_int64),
        ("hbm_bytes_est", C.c_int64),
        ("kernel_ns", C.c_int64),
        ("exec_ns", C.c_int64),
        ("load_ns", C.c_int64),
        ("decomp_ns", C.c_int64),
        ("cache_hit_bytes", C.c_int64),
    ]


class GpuqDecompPage(C.Structure):
    """Test support (gpuq_test_decompress): one compressed block."""
    _fields_ = [
        ("codec", C.c_int32),
        ("comp", C.c_void_p),
        ("comp_len", C.c_uint32),
        ("uncomp_len", C.c_uint32),
    ]


class GpuqDecompStats(C.Structure):
    """Test support: the path a page took and its record counts."""
    _fields_ = [("mode", C.c_int32)] + [
        (n, C.c_uint32) for n in (
            "n_seq", "n_segs", "n_big", "n_lit_lane", "n_lit_wave", "n_inl",
            "n_res_lane", "n_res_wave", "n_pieces", "n_backrefs", "n_far",
            "n_tile", "n_tile_rec")
    ]


# gpuq_test_decompress plan modes / flags and per-page paths (include/gpuq.h)
DECOMP_MODES = {"auto": 0, "segment": 1, "litpar": 2, "fallback": 3}
DECOMP_HOST_ONLY = 0x100
DECOMP_HOST_REPLAY = 0x200
DECOMP_PATHS = ("segment", "litpar", "fallback", "raw", "host_image")
CODECS = {"uncompressed": 0, "snappy": 1, "lz4_raw": 7}

OPS = {"eq": 0, "ne": 1, "lt": 2, "le": 3, "gt": 4, "ge": 5, "between": 6, "contains": 7,
       "icontains": 8, "starts_with": 9, "ends_with": 10, "not_contains": 11,
       "not_icontains": 12, "not_starts_with": 13, "not_ends_with": 14,
       "is_null": 15, "is_not_null": 16,
       "like": 17, "not_like": 18, "ilike": 19, "not_ilike": 20}
# the LIKE-family string ops and the literal-free null ops (include/gpuq.h)
STR_OPS = ("contains", "icontains", "starts_with", "ends_with", "not_contains",
           "not_icontains", "not_starts_with", "not_ends_with")
# general patterns: the literal is the SQL pattern as written ('%', '_',
# backslash escape), not an unescaped byte string
PATTERN_OPS = ("like", "not_like", "ilike", "not_ilike")
NULL_OPS = ("is_null", "is_not_null")
# gpuq_node_kind, and the query-IR keys of the two group kinds
NODE_KINDS = {"leaf": 0, "and": 1, "or": 2}
# gpuq_test_mask_ops (test support): ops, margin and sentinel of include/gpuq.h
MASK_OPS = {"or_reset": 0, "and": 1}
MASK_TEST_MARGIN = 32
MASK_TEST_SENTINEL = 0xA5
AGGS = {"count_star": 0, "count": 1, "sum": 2, "min": 3, "max": 4,
        "count_distinct": 5}

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"libgpuq.so not built at {LIB_PATH} — run __graft_entry__.build(). "
            "parseable_amd has no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    lib.gpuq_session_create.restype = C.c_void_p
    lib.gpuq_session_create.argtypes = [C.c_uint64]
    lib.gpuq_session_destroy.argtypes = [C.c_void_p]
    lib.gpuq_last_error.restype = C.c_char_p
    lib.gpuq_last_error.argtypes = [C.c_void_p]
    lib.gpuq_device_count.restype = C.c_int32
    lib.gpuq_plan_build_from_stream.restype = C.c_void_p
    lib.gpuq_plan_build_from_stream.argtypes = [
        C.c_void_p, C.c_char_p,
        C.POINTER(C.c_char_p), C.c_int32,
        C.POINTER(GpuqPred), C.c_int32,
        C.POINTER(C.c_char_p), C.c_int32,
        C.POINTER(GpuqAgg), C.c_int32,
        C.c_int64, C.POINTER(C.c_int64),
    ]
    lib.gpuq_plan_build.restype = C.c_void_p
    lib.gpuq_plan_build.argtypes = [
        C.c_void_p,
        C.POINTER(GpuqFile), C.c_int32,
        C.POINTER(C.c_char_p), C.c_int32,
        C.POINTER(GpuqPred), C.c_int32,
        C.POINTER(C.c_char_p), C.c_int32,
        C.POINTER(GpuqAgg), C.c_int32,
        C.c_int64,
    ]
    # the *_where entry points: the same argument lists + (nodes, n_nodes)
    lib.gpuq_plan_build_from_stream_where.restype = C.c_void_p
    lib.gpuq_plan_build_from_stream_where.argtypes = (
        lib.gpuq_plan_build_from_stream.argtypes
        + [C.POINTER(GpuqWhereNode), C.c_int32])
    lib.gpuq_plan_build_where.restype = C.c_void_p
    lib.gpuq_plan_build_where.argtypes = (
        lib.gpuq_plan_build.argtypes + [C.POINTER(GpuqWhereNode), C.c_int32])
    # the *_filtered entry points: the *_where lists + (filters, n_filters)
    lib.gpuq_plan_build_from_stream_filtered.restype = C.c_void_p
    lib.gpuq_plan_build_from_stream_filtered.argtypes = (
        lib.gpuq_plan_build_from_stream_where.argtypes
        + [C.POINTER(GpuqAggFilter), C.c_int32])
    lib.gpuq_plan_build_filtered.restype = C.c_void_p
    lib.gpuq_plan_build_filtered.argtypes = (
        lib.gpuq_plan_build_where.argtypes
        + [C.POINTER(GpuqAggFilter), C.c_int32])
    lib.gpuq_test_mask_ops.restype = C.c_int32
    lib.gpuq_test_mask_ops.argtypes = [
        C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
        C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
    ]
    lib.gpuq_plan_partition_count.restype = C.c_int32
    lib.gpuq_plan_partition_count.argtypes = [C.c_void_p]
    lib.gpuq_plan_load.restype = C.c_int32
    lib.gpuq_plan_load.argtypes = [C.c_void_p, C.c_int32]
    lib.gpuq_plan_execute.restype = C.c_int32
    lib.gpuq_plan_execute.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.gpuq_plan_metrics.restype = C.c_int32
    lib.gpuq_plan_metrics.argtypes = [C.c_void_p, C.POINTER(GpuqMetrics)]
    lib.gpuq_plan_destroy.argtypes = [C.c_void_p]
    lib.gpuq_test_decompress.restype = C.c_int32
    lib.gpuq_test_decompress.argtypes = [
        C.c_void_p, C.POINTER(GpuqDecompPage), C.c_int32, C.c_int32, C.c_int32,
        C.c_uint8, C.c_void_p, C.c_uint64,
        C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
        C.POINTER(GpuqDecompStats), C.POINTER(C.c_int32),
    ]
    lib.gpuq_test_like_match.restype = C.c_int32
    lib.gpuq_test_like_match.argtypes = [
        C.c_char_p, C.c_uint32, C.c_int32, C.c_char_p, C.c_uint32]
    _lib = lib
    return lib


def device_count() -> int:
    return load().gpuq_device_count()


def decompress_pages(pages, mode="auto", raw_lead=0, host=None, session=None,
                     sentinel=0xA5):
    """Test support: run the page-decompression planner (and, with a session
    handle, the decompress kernels) on compressed blocks.

    pages: [(codec name, compressed bytes, uncompressed length)].
    host: None (device; needs `session`, a gpuq_ctx handle), "decode" (the
    host scalar decoders) or "replay" (serial host replay of the planned
    records). Returns (arena bytes, [stats dict per page], guard_len, d_err);
    raises RuntimeError with the library's message when it refuses."""
    lib = load()
    n = len(pages)
    arr = (GpuqDecompPage * max(n, 1))()
    keep = []
    cap = 16384 + 64
    for i, (codec, comp, uncomp) in enumerate(pages):
        buf = C.create_string_buffer(bytes(comp), max(len(comp), 1))
        keep.append(buf)
        arr[i] = GpuqDecompPage(CODECS[codec], C.addressof(buf), len(comp), uncomp)
        cap += (uncomp + 15) & ~15
    flags = DECOMP_MODES[mode] | {None: 0, "decode": DECOMP_HOST_ONLY,
                                  "replay": DECOMP_HOST_REPLAY}[host]
    out = C.create_string_buffer(cap)
    arena_len, guard_len, d_err = C.c_uint64(), C.c_uint64(), C.c_int32()
    stats = (GpuqDecompStats * max(n, 1))()
    rc = lib.gpuq_test_decompress(
        session if host is None else None, arr, n, raw_lead, flags, sentinel,
        out, cap, C.byref(arena_len), C.byref(guard_len), stats, C.byref(d_err))
    if rc != 0:
        msg = lib.gpuq_last_error(session if host is None else None)
        raise RuntimeError(msg.decode(errors="replace"))
    st = []
    for i in range(n):
        d = {f: getattr(stats[i], f) for f, _ in GpuqDecompStats._fields_}
        d["mode"] = DECOMP_PATHS[d["mode"]]
        st.append(d)
    return out.raw[:arena_len.value], st, guard_len.value, d_err.value


def mask_ops(session, op, a, b, a_lead=0, b_lead=0):
    """Test support: run k_mask_or_reset ("or_reset": a |= b, b = 1) or
    k_mask_and ("and": a &= b) on two equally long byte strings placed at
    device addresses with (address % 16) == lead. `session` is a gpuq_ctx
    handle. Returns (out_a, out_b): the whole device buffers, MASK_TEST_MARGIN
    sentinel bytes + lead sentinel bytes before the data and MASK_TEST_MARGIN
    after it."""
    lib = load()
    a, b = bytes(a), bytes(b)
    if len(a) != len(b):
        raise ValueError("mask_ops: a and b differ in length")
    n = len(a)
    ba = C.create_string_buffer(a, max(n, 1))
    bb = C.create_string_buffer(b, max(n, 1))
    out_a = C.create_string_buffer(2 * MASK_TEST_MARGIN + a_lead + n)
    out_b = C.create_string_buffer(2 * MASK_TEST_MARGIN + b_lead + n)
    rc = lib.gpuq_test_mask_ops(session, MASK_OPS[op], C.addressof(ba),
                                C.addressof(bb), n, a_lead, b_lead,
                                C.addressof(out_a), C.addressof(out_b))
    if rc != 0:
        raise RuntimeError(lib.gpuq_last_error(session).decode(errors="replace"))
    return out_a.raw, out_b.raw


def like_match(pattern: bytes, fold: bool, value: bytes) -> int:
    """Test support: compile `pattern` (GPUQ_LIKE syntax; fold = the ILIKE
    rules) and run the matcher the kernels share on `value`. 1 / 0, or -1 when
    the pattern does not compile."""
    return load().gpuq_test_like_match(bytes(pattern), len(pattern),
                                       1 if fold else 0, bytes(value),
                                       len(value))
