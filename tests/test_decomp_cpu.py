"""Page decompression without a GPU: the host scalar decoders, the host
walks (through a serial host replay of the records they plan) and the
path-coverage of the named cases, all through gpuq_test_decompress in its
host-only modes. The kernels themselves are tests/test_gpu_decomp.py.

The replay test subsumes the old manual scripts/lz4_litpar_check.cpp: it
applies the literal, inline, resolved and windowed records of every plan
(not only litpar) the way the kernels would and compares with the reference
decoder, on built streams instead of whatever a parquet file holds."""

import subprocess

import pytest

from tests import decomp_common as dc
from tests.conftest import REPO_ROOT


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", f"{REPO_ROOT}/parseable_amd/csrc"],
                   check=True, capture_output=True)


# ---- builders ---------------------------------------------------------
def test_lz4_block_builder_follows_the_block_format():
    lit = bytes(range(20))
    blk = dc.lz4_block([(lit, 3, 300), (b"", 1, 4), (b"ab", 2, 19)], b"x" * 12)
    # token 0xFF, literal extension 5, 20 literals, offset 3, extensions
    # 255 + 26 (300 - 4 - 15 = 281); then token 0x00, offset 1
    assert blk[:2] == b"\xff\x05" and blk[22:26] == b"\x03\x00\xff\x1a"
    assert blk[26:29] == b"\x00\x01\x00"
    assert blk[29:30] == b"\x2f" and blk[34:35] == b"\x00"   # 19 - 4 = 15 + 0
    assert len(dc.lz4_decode(blk, 20 + 300 + 4 + 2 + 19 + 12)) == 357
    with pytest.raises(AssertionError):
        dc.lz4_block([(lit, 3, 4)], b"x" * 11)    # end rule: tail too short


def test_length_extension_edges_are_in_the_cases():
    """15, 15+255 and 15+255+255 for literals; the same +4 for matches"""
    assert {15, 270, 525} <= set(dc.LONG_LIT_LENS)
    blk = dc.lz4_block([(b"a" * 16, 1, 19), (b"", 1, 274), (b"", 1, 529)],
                       b"t" * 12)
    assert blk[20:21] == b"\x00" and blk[24:26] == b"\xff\x00"
    assert blk[29:32] == b"\xff\xff\x00"
    assert len(dc.lz4_decode(blk, 16 + 19 + 274 + 529 + 12)) == 850


def test_snappy_builder_forms():
    b = dc.SnappyBuilder(1)
    b.lit(b"a" * 5, 0).lit(b"b" * 5, 1).lit(b"c" * 5, 2).lit(b"d" * 5, 3)
    b.copy(5, 4, 1).copy(7, 64, 2).copy(9, 1, 4)
    blk = b.finish()
    assert blk[0] == 5 * 4 + 4 + 64 + 1
    assert blk[1] == 4 << 2 and blk[7] == 60 << 2 and blk[8] == 4
    assert blk[14] == 61 << 2 and blk[22] == 62 << 2
    assert blk[31:33] == bytes([1, 5])                      # copy1 len 4 off 5
    assert blk[33:36] == bytes([2 | 63 << 2, 7, 0])         # copy2
    assert blk[36:41] == bytes([3, 9, 0, 0, 0])             # copy4 len 1
    assert len(dc.snappy_decode(blk)) == blk[0]


# ---- host decoders and host walks vs the reference --------------------
@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_host_decoders_match_reference(name):
    pages = dc.case(name)
    arena, st, guard, err = dc.run_case(pages, "auto", host="decode")
    assert err == 0 and guard >= 16384
    dc.check_arena(f"{name}/host-decode", pages, arena, st, guard)


@pytest.mark.parametrize("mode", dc.MODES)
@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_host_replay_of_planned_records_matches_reference(name, mode):
    """the plan of every mode, applied serially on the host in launch order
    onto a sentinel-filled arena, yields the reference bytes and nothing
    else: checks lz4_walk (segment and litpar), snappy_walk and the record
    building, with the source alignment varied"""
    pages = dc.case(name)
    want_stats = dc.run_case(pages, mode, host="decode")[1]
    for lead in (0, 5):
        arena, st, guard, _ = dc.run_case(pages, mode, raw_lead=lead,
                                          host="replay", sentinel=0x3C)
        assert st == want_stats
        dc.check_arena(f"{name}/{mode}/lead{lead}/replay", pages, arena, st,
                       guard, sentinel=0x3C)


def test_stats_are_consistent_with_the_streams():
    for name in dc.CASE_NAMES:
        pages = dc.case(name)
        for mode in dc.MODES:
            for p, s in zip(pages, dc.run_case(pages, mode, host="decode")[1]):
                if s["mode"] in ("raw", "host_image"):
                    continue
                spans = list(dc._snappy_spans(p.comp) if p.codec == "snappy"
                             else dc._lz4_spans(p.comp))
                lits = [x for x in spans if x[0] == "literal"]
                matches = [x for x in spans if x[0] == "match"]
                if s["mode"] == "litpar":
                    # one literal record per literal run, one match record
                    # per match, split at 256 bytes
                    assert s["n_lit_lane"] == sum(x[2] <= 256 for x in lits)
                    assert s["n_lit_wave"] == sum(x[2] > 256 for x in lits)
                    assert s["n_res_wave"] == sum(x[2] > 256 for x in matches)
                    assert (s["n_inl"] + s["n_res_lane"]
                            == sum(x[2] <= 256 for x in matches))
                    assert s["n_segs"] == s["n_backrefs"] == 0
                else:
                    assert s["n_lit_lane"] == s["n_lit_wave"] == s["n_inl"] == 0
                    # a match longer than a segment makes its sequence `big`
                    assert s["n_segs"] > s["n_big"] >= sum(
                        x[2] > dc.SEG_MAX for x in matches)
                if s["mode"] == "fallback":
                    assert s["n_res_lane"] == s["n_res_wave"] == s["n_pieces"] == 0
                    assert s["n_far"] <= s["n_backrefs"] <= len(matches)
                    assert s["n_far"] >= sum(x[2] > dc.SEG_MAX for x in matches)


# ---- path coverage: every named case reaches the path it is named for --
def _stats(name, mode):
    return dc.run_case(dc.case(name), mode, host="decode")[1]


def test_dense_short_reaches_litpar_inline_and_lane():
    (s,) = _stats("dense_short", "auto")
    assert s["mode"] == "litpar" and s["n_seq"] >= 3000
    assert s["n_lit_lane"] > 0 and s["n_inl"] > 0 and s["n_res_lane"] > 0
    (g,) = _stats("dense_short", "segment")
    # the segment plan of the same page: deferred matches resolve through
    # more than one piece each on average
    assert g["mode"] == "segment" and g["n_segs"] >= 4
    assert g["n_res_lane"] > 0 and g["n_pieces"] > g["n_res_lane"]


def test_periods_inline_every_period_and_hand_257_to_the_wave_kernel():
    (s,) = _stats("periods", "litpar")
    n_short = sum(ml <= 256 for ml in dc.PERIOD_LENS)
    assert s["mode"] == "litpar"
    # each source lies inside one literal run; offsets 1..8 give a pattern of
    # min(off, len) <= 8 bytes: inlined. Offset 9 inlines only len <= 8 and
    # sends the 9-byte patterns (len 9, 255, 256) to the lane resolver
    assert s["n_inl"] == 8 * n_short + sum(ml <= 8 for ml in dc.PERIOD_LENS)
    assert s["n_res_lane"] == sum(8 < ml <= 256 for ml in dc.PERIOD_LENS) == 3
    assert s["n_res_wave"] == 9 * (len(dc.PERIOD_LENS) - n_short) == 9
    (g,) = _stats("periods", "auto")
    assert g["mode"] == "segment"       # in-segment overlapping copies


def test_long_matches_reach_the_wave_resolver_in_both_plans():
    (g,) = _stats("long_matches", "auto")
    assert g["mode"] == "segment" and g["n_res_wave"] > 0
    (s,) = _stats("long_matches", "litpar")
    assert s["mode"] == "litpar"
    assert s["n_res_wave"] == len(dc.LONG_MATCH_LENS)


def test_long_literals_reach_the_wave_literal_kernel():
    (s,) = _stats("long_literals", "litpar")
    assert s["mode"] == "litpar"
    assert s["n_lit_wave"] == sum(n > 256 for n in dc.LONG_LIT_LENS)
    assert s["n_lit_lane"] > 0
    (g,) = _stats("long_literals", "auto")
    assert g["mode"] == "segment" and g["n_big"] == 0


def test_refill_edges_run_in_the_segment_kernel():
    st = _stats("refill_edges", "auto")
    assert all(s["mode"] == "segment" for s in st)
    n_probe = 3 * len(dc._PROBE)
    assert all(s["n_segs"] == 1 and s["n_big"] == 0 for s in st[:n_probe])
    assert all(s["n_big"] == 1 for s in st[n_probe:]) and len(st) == n_probe + 9
    # the probed field really sits on the probed compressed offset
    pages = dc.case("refill_edges")
    i = 0
    for field, (nlit, pos) in dc._PROBE.items():
        for x in (4095, 4096, 4097):
            comp = pages[i].comp
            start = x - pos
            if nlit < 15:
                assert comp[start] == (nlit << 4) | 15
                assert comp[start + 4:start + 8] == b"\x09\x00\xff\x1a"
            else:
                assert comp[start] == 0xFF
            i += 1


def test_giant_sequences_make_big_segments():
    st = _stats("giant", "auto")
    assert [s["mode"] for s in st] == ["segment"] * 4
    assert [s["n_big"] for s in st] == [1, 1, 1, 2]
    assert all(s["n_res_lane"] + s["n_res_wave"] > 0 for s in st)
    fb = _stats("giant", "fallback")
    assert all(s["n_far"] > 0 for s in fb[1:])


def test_organic_fallback_needs_no_knob_and_takes_both_resolver_branches():
    (s,) = _stats("organic_fallback", "auto")
    assert s["mode"] == "fallback" and s["n_big"] == 2
    assert s["n_far"] >= 9
    assert s["n_backrefs"] - s["n_far"] >= 48     # 2 x 12 x 2 near records


def test_segment_straddle_defers_across_segment_starts():
    (g,) = _stats("segment_straddle", "segment")
    assert g["mode"] == "segment" and g["n_segs"] == 4
    # 2 straddlers + source at seg_start - 1 + chain of 7 + 3 x 2 + 3
    assert g["n_res_lane"] + g["n_res_wave"] >= 19 and g["n_res_wave"] >= 3
    assert g["n_pieces"] > g["n_res_lane"] + g["n_res_wave"]   # multi-piece
    (f,) = _stats("segment_straddle", "fallback")
    assert f["n_far"] == 4                 # offsets 8191..8193, 8000 + 193


def test_stored_raw_and_tiny_pages():
    st = _stats("stored_raw", "auto")
    assert all(s["mode"] == "raw" and s["n_segs"] == 1 for s in st)
    assert len(st) == 2 * len(dc.RAW_SIZES)
    assert [len(p.ref) for p in dc.case("tiny")] == [1, 12, 26]
    assert [s["n_seq"] for s in _stats("tiny", "auto")] == [1, 1, 2]


def test_snappy_pages_ride_the_litpar_records():
    forms, overlap = _stats("snappy_forms", "auto")
    assert forms["mode"] == overlap["mode"] == "litpar"
    assert forms["n_lit_wave"] >= 4 and forms["n_lit_lane"] > 0
    assert overlap["n_inl"] == 8 * 11      # every offset 1..8 pattern inlined
    (m,) = _stats("snappy_max_pieces", "auto")
    # A snappy copy has <= 64 bytes and every piece covers >= 1 byte, so a
    # record never needs more than 64 pieces and snappy_walk's explosion
    # limit (> 64) — the host-image path — is out of reach of any valid
    # stream; this page reaches the maximum, one piece per byte
    assert m["mode"] == "litpar"
    assert m["n_pieces"] == 64 * m["n_res_lane"] and m["n_res_lane"] == 60


def test_every_decompress_kernel_and_branch_is_reached_by_a_named_case():
    seen = {k: 0 for k in ("n_segs", "n_big", "n_lit_lane", "n_lit_wave",
                           "n_inl", "n_res_lane", "n_res_wave", "n_far",
                           "near", "raw")}
    for name in dc.NAMED:
        for mode in dc.MODES:
            for s in _stats(name, mode):
                for k in seen:
                    if k in s:
                        seen[k] += s[k]
                seen["near"] += s["n_backrefs"] - s["n_far"]
                seen["raw"] += s["mode"] == "raw"
    assert all(v > 0 for v in seen.values()), seen


# ---- malformed streams: an error, never a crash -----------------------
def _lz4_bad():
    ok = dc.lz4_block([(b"abcdefgh", 3, 300), (b"q" * 20, 5, 6)], b"t" * 12)
    n = 8 + 300 + 20 + 6 + 12
    # layout: 0 token, 1..8 lits, 9..10 offset, 11..12 ml ext, 13 token,
    # 14 lit ext, 15..34 lits, 35..36 offset, 37 last token
    return {
        "truncated_in_token": (ok[:14], n),          # token promises literals
        "truncated_in_literal_length": (ok[:14] + b"\xff", n),
        "truncated_in_match_length": (ok[:12], n),
        "truncated_in_offset": (ok[:10], n),
        "offset_zero": (ok[:9] + b"\x00\x00" + ok[11:], n),
        "offset_before_output": (ok[:9] + b"\x09\x00" + ok[11:], n),
        "literal_overrun": (ok[:37] + b"\xf0\x10" + ok[38:], n),
        "literal_overrun_output": (ok, n - 1),
        "match_overrun": (ok[:35] + b"\x05\x00", 8 + 300 + 20 + 5),
        "size_mismatch_short": (ok, n + 1),
        "size_mismatch_trailing": (ok[:37] + b"\x10t", n),
    }


def _snappy_bad():
    b = dc.SnappyBuilder(5)
    b.lit(30).copy(7, 20, 2).lit(20, 1).copy(3, 9, 1).copy(50, 4, 4).lit(5)
    ok = b.finish()
    n = b.d
    assert n < 128      # one preamble byte
    # layout: 0 preamble, 1 tag, 2..31 lits, 32 copy2 tag, 33..34 offset,
    # 35 literal tag, 36 length byte, 37..56 lits, 57 copy1, 59 copy4 tag,
    # 60..63 offset, 64 literal tag
    return {
        "preamble_11_bytes": (b"\x80" * 10 + b"\x00" + ok[1:], n),
        "preamble_64_bytes": (b"\xff" * 64 + b"\x00" + ok[1:], n),
        "preamble_unterminated": (b"\x80" * 5, n),
        "preamble_disagrees": (ok, n + 1),
        "preamble_disagrees_low": (bytes([n - 1]) + ok[1:], n),
        "truncated_in_literal_length": (ok[:36], n),
        "truncated_in_literal": (ok[:20], n),
        "truncated_in_offset": (ok[:34], n),
        "truncated_in_copy4": (ok[:62], n),
        "offset_zero": (ok[:33] + b"\x00\x00" + ok[35:], n),
        "offset_before_output": (ok[:33] + b"\x1f\x00" + ok[35:], n),
        "match_overrun": (ok + b"\xfe\x01\x00", n),
        "literal_overrun": (ok + b"\x10abcde", n),
    }


_BAD = ([("lz4_raw", k, v) for k, v in _lz4_bad().items()]
        + [("snappy", k, v) for k, v in _snappy_bad().items()])


@pytest.mark.parametrize("codec,what,stream", _BAD,
                         ids=[f"{c}-{k}" for c, k, _ in _BAD])
def test_malformed_stream_is_rejected(codec, what, stream):
    comp, uncomp = stream
    assert len(comp) != uncomp          # else it would count as stored raw
    decode = dc.lz4_decode if codec == "lz4_raw" else dc.snappy_decode
    with pytest.raises(ValueError):     # the reference agrees it is malformed
        ref = decode(comp, uncomp) if codec == "lz4_raw" else decode(comp)
        if len(ref) != uncomp:
            raise ValueError("size mismatch")
    good = dc.case("tiny")[2]
    for mode in dc.MODES:
        for host in ("decode", "replay"):
            with pytest.raises(RuntimeError) as ei:
                dc.run_case([good, dc.Page(codec, comp, b"\0" * uncomp)], mode,
                            host=host)
            assert str(ei.value) not in ("", "null ctx")


def test_entry_rejects_bad_arguments():
    good = dc.case("tiny")
    with pytest.raises(RuntimeError):
        dc.run_case(good, "auto", raw_lead=16, host="decode")
    with pytest.raises(RuntimeError, match="session"):
        dc.run_case(good, "auto", host=None, session=None)
    with pytest.raises(RuntimeError, match="codec"):
        from parseable_amd import _lib
        saved = dict(_lib.CODECS)
        _lib.CODECS["gzip"] = 2
        try:
            dc.run_case([dc.Page("gzip", b"abc", b"abc")], host="decode")
        finally:
            _lib.CODECS.clear()
            _lib.CODECS.update(saved)
