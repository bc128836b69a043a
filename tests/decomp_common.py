"""Compressed-page builders, byte-loop reference decoders and the named
cases of the decompression differential (tests/test_decomp_cpu.py,
tests/test_gpu_decomp.py). No GPU import.

A case is a list of pages; a page is (codec name, compressed block,
reference image). Every block is built sequence by sequence so the edges of
the formats are chosen on purpose, decoded by the plain Python decoder below
(the reference) and cross-checked against pyarrow's liblz4 / snappy: a block
on which the two disagree is a bug in the builder, not a test case.

Constants mirrored from the kernels (parseable_amd/csrc/kernels.hip):
SEG_MAX 8192 output bytes per segment, LZ4_IN 4096-byte input window,
BR_WIN 16384 (far branch when off + len > BR_WIN / 2), 256 = lane / wave
record split, 8 = longest host-inlined pattern."""

from __future__ import annotations

import random
from collections import namedtuple

SEG_MAX = 8192
LZ4_IN = 4096
BR_FAR = 8192

Page = namedtuple("Page", "codec comp ref")


# --------------------------------------------------------------------
# reference decoders (plain byte loops; raise ValueError when malformed)
# --------------------------------------------------------------------
def _copy_match(out: bytearray, off: int, ml: int) -> None:
    if off <= 0 or off > len(out):
        raise ValueError("bad offset")
    for _ in range(ml):          # byte by byte: overlap repeats the pattern
        out.append(out[-off])


def lz4_decode(block: bytes, uncomp: int) -> bytes:
    out = bytearray()
    s, n = 0, len(block)
    while s < n:
        token = block[s]
        s += 1
        lit = token >> 4
        if lit == 15:
            while True:
                if s >= n:
                    raise ValueError("eof in literal length")
                b = block[s]
                s += 1
                lit += b
                if b != 255:
                    break
        if s + lit > n:
            raise ValueError("literal overrun")
        out += block[s:s + lit]
        s += lit
        if s >= n:
            break
        if s + 2 > n:
            raise ValueError("eof in offset")
        off = block[s] | (block[s + 1] << 8)
        s += 2
        ml = token & 15
        if ml == 15:
            while True:
                if s >= n:
                    raise ValueError("eof in match length")
                b = block[s]
                s += 1
                ml += b
                if b != 255:
                    break
        _copy_match(out, off, ml + 4)
        if len(out) > uncomp:
            raise ValueError("output overrun")
    if len(out) != uncomp:
        raise ValueError("size mismatch")
    return bytes(out)


def snappy_decode(block: bytes) -> bytes:
    s, n, ulen, sh = 0, len(block), 0, 0
    while True:
        if s >= n or sh > 63:
            raise ValueError("bad preamble")
        b = block[s]
        s += 1
        ulen |= (b & 0x7F) << sh
        if not b & 0x80:
            break
        sh += 7
    out = bytearray()
    while s < n:
        tag = block[s]
        s += 1
        kind = tag & 3
        if kind == 0:
            ln = (tag >> 2) + 1
            if ln > 60:
                extra = ln - 60
                if s + extra > n:
                    raise ValueError("eof in literal length")
                ln = int.from_bytes(block[s:s + extra], "little") + 1
                s += extra
            if s + ln > n:
                raise ValueError("literal overrun")
            out += block[s:s + ln]
            s += ln
            continue
        if kind == 1:
            ml = ((tag >> 2) & 7) + 4
            if s + 1 > n:
                raise ValueError("eof in offset")
            off = ((tag >> 5) << 8) | block[s]
            s += 1
        else:
            nb = 2 if kind == 2 else 4
            ml = (tag >> 2) + 1
            if s + nb > n:
                raise ValueError("eof in offset")
            off = int.from_bytes(block[s:s + nb], "little")
            s += nb
        _copy_match(out, off, ml)
    if len(out) != ulen:
        raise ValueError("size mismatch")
    return bytes(out)


# --------------------------------------------------------------------
# builders
# --------------------------------------------------------------------
def _lz4_len_ext(n: int) -> bytes:
    """extension bytes for a length field whose nibble is 15 (n >= 15)"""
    n -= 15
    return b"\xff" * (n // 255) + bytes([n % 255])


class Lz4Builder:
    """LZ4 block, one sequence at a time. `s` / `d` are the compressed and
    decompressed lengths so far, so a recipe can place a field at an exact
    compressed offset or a match at an exact output offset."""

    def __init__(self, seed: int):
        self.rng = random.Random(seed)
        self.comp = bytearray()
        self.d = 0

    @property
    def s(self) -> int:
        return len(self.comp)

    def rand(self, n: int) -> bytes:
        return self.rng.randbytes(n)

    def seq(self, lit, off: int, ml: int) -> "Lz4Builder":
        """literals (bytes, or a count of random bytes), then a match"""
        if isinstance(lit, int):
            lit = self.rand(lit)
        assert ml >= 4 and 1 <= off <= 65535 and off <= self.d + len(lit)
        self.comp.append((min(len(lit), 15) << 4) | min(ml - 4, 15))
        if len(lit) >= 15:
            self.comp += _lz4_len_ext(len(lit))
        self.comp += lit
        self.comp += bytes([off & 255, off >> 8])
        if ml - 4 >= 15:
            self.comp += _lz4_len_ext(ml - 4)
        self.d += len(lit) + ml
        return self

    def finish(self, tail=12, strict: bool = True) -> bytes:
        """the last sequence: literals only. The block format's end rules
        (>= 5 trailing literals, last match ends >= 12 bytes before the end)
        hold when the tail has >= 12 bytes; strict=False is for blocks too
        small to hold a match at all."""
        if isinstance(tail, int):
            tail = self.rand(tail)
        assert not strict or len(tail) >= 12
        self.comp.append(min(len(tail), 15) << 4)
        if len(tail) >= 15:
            self.comp += _lz4_len_ext(len(tail))
        self.comp += tail
        self.d += len(tail)
        return bytes(self.comp)


def lz4_block(seqs, tail, strict: bool = True) -> bytes:
    """LZ4 block from [(literal bytes, offset, match length)] + tail literals"""
    b = Lz4Builder(0)
    for lit, off, ml in seqs:
        b.seq(bytes(lit), off, ml)
    return b.finish(bytes(tail), strict)


def _uvarint(n: int) -> bytes:
    out = bytearray()
    while n >= 0x80:
        out.append((n & 0x7F) | 0x80)
        n >>= 7
    out.append(n)
    return bytes(out)


class SnappyBuilder:
    def __init__(self, seed: int):
        self.rng = random.Random(seed)
        self.body = bytearray()
        self.d = 0

    def rand(self, n: int) -> bytes:
        return self.rng.randbytes(n)

    def lit(self, data, extra: int | None = None) -> "SnappyBuilder":
        """literal; extra = number of length bytes after the tag (0..3),
        default the shortest form"""
        if isinstance(data, int):
            data = self.rand(data)
        n = len(data) - 1
        assert n >= 0
        if extra is None:
            extra = 0 if n < 60 else (n.bit_length() + 7) // 8
        if extra == 0:
            assert n < 60
            self.body.append(n << 2)
        else:
            assert 1 <= extra <= 4 and n < (1 << (8 * extra))
            self.body.append((59 + extra) << 2)
            self.body += n.to_bytes(extra, "little")
        self.body += data
        self.d += len(data)
        return self

    def copy(self, off: int, ml: int, form: int | None = None) -> "SnappyBuilder":
        """copy with a 1-, 2- or 4-byte offset (form), default the shortest"""
        assert 1 <= off <= self.d
        if form is None:
            form = 1 if (4 <= ml <= 11 and off < 2048) else 2 if off < 65536 else 4
        if form == 1:
            assert 4 <= ml <= 11 and off < 2048
            self.body.append(1 | ((ml - 4) << 2) | ((off >> 8) << 5))
            self.body.append(off & 255)
        else:
            assert 1 <= ml <= 64 and form in (2, 4) and off < (1 << (8 * form))
            self.body.append((2 if form == 2 else 3) | ((ml - 1) << 2))
            self.body += off.to_bytes(form, "little")
        self.d += ml
        return self

    def finish(self) -> bytes:
        return _uvarint(self.d) + bytes(self.body)


# --------------------------------------------------------------------
# second opinion + page construction
# --------------------------------------------------------------------
def _second_opinion(codec: str, comp: bytes, uncomp: int) -> bytes:
    import pyarrow as pa

    return pa.Codec(codec).decompress(comp, uncomp).to_pybytes()


def lz4_page(comp: bytes, uncomp: int) -> Page:
    ref = lz4_decode(comp, uncomp)
    assert _second_opinion("lz4_raw", comp, uncomp) == ref, "builder bug (lz4)"
    return Page("lz4_raw", comp, ref)


def snappy_page(comp: bytes) -> Page:
    ref = snappy_decode(comp)
    assert _second_opinion("snappy", comp, len(ref)) == ref, "builder bug (snappy)"
    return Page("snappy", comp, ref)


def _done(b: Lz4Builder, tail=12, strict=True) -> Page:
    comp = b.finish(tail, strict)
    return lz4_page(comp, b.d)


# --------------------------------------------------------------------
# named cases
# --------------------------------------------------------------------
def dense_short(seed=101, n=3000) -> list:
    """~3000 sequences, literals 0..5, offsets 1..39, matches 4..11"""
    b = Lz4Builder(seed)
    b.seq(40, 17, 6)
    r = b.rng
    for _ in range(n):
        b.seq(r.randint(0, 5), r.randint(1, 39), r.randint(4, 11))
    return [_done(b)]


PERIOD_LENS = (4, 5, 7, 8, 9, 255, 256, 257)


def periods() -> list:
    """every offset 1..8 (and 9) x match lengths 4, 5, 7, 8, 9, 255, 256, 257;
    the source of each match lies inside the 9..14 literals right before it"""
    b = Lz4Builder(102)
    for off in range(1, 10):         # 9: one past the inline limit
        for ml in PERIOD_LENS:
            b.seq(b.rng.randint(9, 14), off, ml)
    return [_done(b)]


LONG_MATCH_LENS = (257, 258, 300, 511, 512, 513, 1000, 1023, 1024, 1025, 2047,
                   2048, 2049, 2999, 3000, 257, 777, 1500, 3000, 270, 525, 2600)


def long_matches() -> list:
    """matches of 257..3000 bytes, offsets 9..200, 4 literals between them:
    after each segment start the literals are shorter than the offset, so
    the match reaches before the segment and is deferred"""
    b = Lz4Builder(103)
    b.seq(210, 100, 40)
    r = b.rng
    for ml in LONG_MATCH_LENS:
        b.seq(4, r.randint(9, 200), ml)
    return [_done(b)]


LONG_LIT_LENS = (15, 16, 269, 270, 271, 524, 525, 526, 255, 256, 257, 1000,
                 2999, 3000, 4095, 4096, 4097, 14, 3000, 780)


def long_literals() -> list:
    """literals of 15..3000(+) bytes, among them exactly 15, 270 and 525 (one,
    two and three length-extension bytes ending in 0)"""
    b = Lz4Builder(104)
    r = b.rng
    for n in LONG_LIT_LENS:
        b.seq(n, r.randint(1, min(20, n)), r.randint(4, 30))
    return [_done(b)]


def _fill_comp(b: Lz4Builder, target_s: int) -> None:
    """short sequences (l <= 14 literals + a 4..6-byte match, l + 3 compressed
    bytes each) until exactly target_s compressed bytes are written"""
    assert b.s == 0 and target_s >= 40
    while target_s - b.s > 34:
        b.seq(14, b.rng.randint(1, 14), b.rng.randint(4, 6))
    r = target_s - b.s - 6           # 12..28 literals over two sequences
    b.seq(r // 2, 1, 4)
    b.seq(r - r // 2, 1, 4)
    assert b.s == target_s, (b.s, target_s)


# field -> (literal count of the probe sequence, byte position of the field
# inside it). Match length 300 = nibble 15 + extension bytes 255, 26.
_PROBE = {
    "token": (3, 0),
    "off_lo": (3, 4),
    "off_hi": (3, 5),
    "ml_ext": (3, 7),            # second match-length extension byte
    "tokenL": (20, 0),           # same with the long-literal parse (lit >= 15)
    "off_loL": (20, 22),
    "off_hiL": (20, 23),
    "ml_extL": (20, 24),
    "lit_ext": (600, 2),         # second of three literal-length bytes
}


def refill_edges() -> list:
    """compressed offsets 4095, 4096 and 4097 of a segment land on a token,
    an offset byte or a length-extension byte (first window refill of
    k_lz4_seg); the same at 8191..8193 inside a `big` segment, whose
    refills happen at multiples of the window"""
    pages = []
    seed = 200
    for field, (nlit, pos) in _PROBE.items():
        for x in (LZ4_IN - 1, LZ4_IN, LZ4_IN + 1):
            seed += 1
            b = Lz4Builder(seed)
            _fill_comp(b, x - pos)
            b.seq(nlit, 9, 300)
            pg = _done(b)
            assert len(pg.ref) <= SEG_MAX        # one segment: seg start = 0
            pages.append(pg)
    # one window later: a single sequence > SEG_MAX output bytes is its own
    # segment; its literal run refills at 4096 and 8192
    for pos, name in ((0, "off_lo"), (1, "off_hi"), (2, "ml_ext")):
        for x in (2 * LZ4_IN - 1, 2 * LZ4_IN, 2 * LZ4_IN + 1):
            seed += 1
            b = Lz4Builder(seed)
            nlit = x - pos - 33          # token + 32 length bytes + literals
            assert 1 + len(_lz4_len_ext(nlit)) == 33
            b.seq(nlit, 100, 300)
            assert b.s - 4 == x - pos    # 2 offset + 2 extension bytes
            pages.append(_done(b))
    return pages


def giant() -> list:
    """single sequences of more than 8192 output bytes (`big` segments)"""
    pages = []
    b = Lz4Builder(301)
    b.seq(20000, 5, 8)                       # literal-heavy
    pages.append(_done(b))
    b = Lz4Builder(302)
    b.seq(10, 1, 30000)                      # match-heavy, offset 1
    pages.append(_done(b))
    b = Lz4Builder(303)
    b.seq(10, 7, 30000)                      # match-heavy, offset 7
    pages.append(_done(b))
    b = Lz4Builder(304)
    b.seq(9000, 3000, 20000)                 # 9000 literals + 20000 match
    b.seq(9, 28000, 9000)                    # far, non-overlapping giant
    pages.append(_done(b))
    return pages


def organic_fallback() -> list:
    """a deferred period-7 run, then an ~8300-byte match from ~9000 bytes
    back across it: its pattern decomposes into > 64 pieces, so the page
    falls back to the serial windowed resolver with no knob set. Then near
    records (window path), far records (off + len > 8192), and near records
    again, among them in-segment matches that read a deferred gap."""
    b = Lz4Builder(401)
    b.seq(16, 7, 9000)               # big sequence: deferred, period 7
    b.seq(700, 9000, 8300)           # big; source crosses the period-7 run
    r = b.rng

    def near(k):
        for _ in range(k):
            b.seq(4, r.randint(300, 900), r.randint(20, 60))   # before seg start
            b.seq(10, r.randint(20, 34), r.randint(8, 30))     # reads that gap
            b.seq(3, r.randint(1, 8), r.randint(4, 300))       # short period
    near(12)
    for off, ml in ((9000, 50), (8150, 100), (8000, 193), (8000, 192),
                    (8191, 4), (8192, 4), (8193, 4), (12000, 5000),
                    (65535 if b.d > 65535 else b.d, 40)):
        b.seq(5, min(off, b.d + 5), ml)
        b.seq(6, r.randint(8, ml + 6), r.randint(6, 20))       # reads the far dst
    near(12)
    return [_done(b)]


def segment_straddle() -> list:
    """sources that straddle a segment start, matches whose source starts one
    byte before / exactly at / one byte after the segment start, offsets of
    8191..8193, and a chain of matches that each read the previous deferred
    match at a shifted offset (transitive gaps)"""
    b = Lz4Builder(501)
    for _ in range(128):             # 128 x 64 output bytes: segment 0 full
        b.seq(60, b.rng.randint(1, 60), 4)
    assert b.d == SEG_MAX
    # segment 1 starts here (seg_start = 8192)
    b.seq(5, 15, 40)                 # source 8182..: straddles, overlapping
    b.seq(50, 120, 60)               # straddles, plain
    for delta in (1, 0, -1):         # source = seg_start - 1 / + 0 / + 1
        rel = b.d + 7 - SEG_MAX      # dst - seg_start of the match below
        b.seq(7, rel + delta, 9)
    prev = 33
    b.seq(4, b.d + 4 - SEG_MAX + 20, prev)     # chain head: deferred
    for shift in (3, 5, 1, 7, 2, 11):          # each reads the one before
        ml = prev + shift
        b.seq(2, prev + 2 - shift, ml)
        prev = ml
    # fill segment 1 exactly, so segment 2 starts at 16384
    while SEG_MAX * 2 - b.d > 200:
        b.seq(60, b.rng.randint(1, 60), 4)
    rest = SEG_MAX * 2 - b.d
    b.seq(rest - 4, 9, 4)
    assert b.d == 2 * SEG_MAX
    for off in (8191, 8192, 8193):
        b.seq(6, off, 10)
        b.seq(6, 8, 300)             # reads the gap just written (period 8)
    # a match that ends exactly on the segment's last byte, then one whose
    # source is the whole previous segment's tail
    while SEG_MAX * 3 - b.d > 300:
        b.seq(30, b.rng.randint(1, 30), 6)
    rest = SEG_MAX * 3 - b.d
    b.seq(rest - 100, rest - 100 + 50, 100)
    assert b.d == 3 * SEG_MAX
    b.seq(1, 8000, 191)              # off + len = 8191
    b.seq(1, 8000, 192)              # 8192: last window-path size
    b.seq(1, 8000, 193)              # 8193: far
    return [_done(b)]


RAW_SIZES = (1, 15, 16, 17, 4097)


def stored_raw() -> list:
    """comp == uncomp and the bytes are no valid block (a 1-byte block cannot
    yield a byte; the others open with a match of offset 0), as a writer
    stores incompressible pages; plus genuinely uncompressed pages"""
    rng = random.Random(601)
    pages = []
    for n in RAW_SIZES:
        data = b"\x5a" if n == 1 else b"\x00\x00\x00" + rng.randbytes(n - 3)
        try:
            lz4_decode(data, n)
        except ValueError:
            pass
        else:
            raise AssertionError("stored-raw bytes decode as a block")
        pages.append(Page("lz4_raw", data, data))
        plain = rng.randbytes(n)
        pages.append(Page("uncompressed", plain, plain))
    return pages


def tiny() -> list:
    pages = []
    b = Lz4Builder(701)
    pages.append(_done(b, 1, strict=False))          # 1 byte
    b = Lz4Builder(702)
    pages.append(_done(b, 12))                       # 12 literals only
    b = Lz4Builder(703)
    b.seq(8, 4, 6)
    pages.append(_done(b, 12))                       # one sequence + tail
    return pages


def snappy_forms() -> list:
    pages = []
    b = SnappyBuilder(801)
    # literal-length forms: 0..3 extra bytes, shortest and padded encodings
    for n, extra in ((1, 0), (60, 0), (61, 1), (5, 1), (256, 1), (257, 2),
                     (7, 2), (65536, 2), (65537, 3), (300, 3)):
        b.lit(n, extra)
        b.copy(b.rng.randint(1, min(b.d, 2047)), b.rng.randint(4, 11), 1)
    # copy forms: 1-, 2- and 4-byte offsets, far and near, len 1..64
    for off, ml, form in ((5, 4, 1), (2047, 11, 1), (2048, 1, 2), (65535, 64, 2),
                          (9, 33, 2), (65536, 64, 4), (100000, 1, 4), (3, 64, 4),
                          (70000, 37, 4)):
        b.lit(b.rng.randint(1, 30))
        b.copy(off, ml, form)
    b.lit(13)
    pages.append(snappy_page(b.finish()))
    # overlapping copies, offset 1..8
    b = SnappyBuilder(802)
    for off in range(1, 9):
        for ml in (4, 5, 7, 8, 9, 11):
            b.lit(b.rng.randint(8, 14))
            b.copy(off, ml, 1)
        for ml in (1, 2, 12, 63, 64):
            b.lit(b.rng.randint(8, 14))
            b.copy(off, ml, 2)
    pages.append(snappy_page(b.finish()))
    return pages


def snappy_max_pieces() -> list:
    """the densest piece decomposition a snappy stream can ask for: 64-byte
    copies whose sources are runs of period-1 and period-2 copies, composed
    three levels deep (one piece per byte)"""
    b = SnappyBuilder(803)
    b.lit(3)
    for _ in range(40):
        b.copy(1, 64, 2)
        b.lit(1)
        b.copy(2, 63, 2)
    for k in range(30):
        b.copy(64 * 20 + k, 64, 2)
        b.copy(64 * 5 + 3 * k + 1, 64, 2)
    b.lit(9)
    return [snappy_page(b.finish())]


# --- seeded random streams: three distributions per codec -------------
RANDOM_SEEDS = tuple(range(9001, 9021))


def random_lz4(seed: int) -> list:
    b = Lz4Builder(seed)
    r = b.rng
    dist = seed % 3
    limit = r.randint(2000, 60000)
    b.seq(r.randint(1, 40), 1, 4)
    while b.d < limit:
        if dist == 0:        # dense-short
            b.seq(r.randint(0, 5), r.randint(1, min(39, b.d)), r.randint(4, 11))
        elif dist == 1:      # long matches, any offset
            b.seq(r.randint(0, 20), r.randint(1, min(b.d, 65535)),
                  r.choice((4, 18, 19, 256, 257, 273, 274, r.randint(4, 3000))))
        else:                # long literals + mixed matches
            b.seq(r.choice((0, 14, 15, 16, 270, 525, r.randint(0, 3000))),
                  r.randint(1, min(b.d, 9000)) if b.d else 1,
                  r.randint(4, 400))
    return [_done(b, r.randint(12, 40))]


def random_snappy(seed: int) -> list:
    b = SnappyBuilder(seed)
    r = b.rng
    dist = seed % 3
    limit = r.randint(2000, 60000)
    b.lit(r.randint(1, 40))
    while b.d < limit:
        if dist == 0:
            b.lit(r.randint(1, 5))
            b.copy(r.randint(1, min(39, b.d)), r.randint(4, 11))
        elif dist == 1:
            if r.random() < 0.3:
                b.lit(r.randint(1, 20))
            b.copy(r.randint(1, b.d), r.randint(1, 64),
                   r.choice((None, 2, 4)))
        else:
            b.lit(r.choice((1, 60, 61, 256, 257, r.randint(1, 3000))),
                  r.choice((None, None, 2, 3)))
            b.copy(r.randint(1, min(b.d, 9000)), r.randint(1, 64))
    return [snappy_page(b.finish())]


NAMED = {
    "dense_short": dense_short,
    "periods": periods,
    "long_matches": long_matches,
    "long_literals": long_literals,
    "refill_edges": refill_edges,
    "giant": giant,
    "organic_fallback": organic_fallback,
    "segment_straddle": segment_straddle,
    "stored_raw": stored_raw,
    "tiny": tiny,
    "snappy_forms": snappy_forms,
    "snappy_max_pieces": snappy_max_pieces,
}

_cache: dict = {}


def case(name: str) -> list:
    """pages of a case, built (and reference-decoded) once per process"""
    if name not in _cache:
        if name == "mixed_arena":
            _cache[name] = [p for n in NAMED for p in case(n)]
        elif name.startswith("rand_lz4_"):
            _cache[name] = random_lz4(int(name[9:]))
        elif name.startswith("rand_snappy_"):
            _cache[name] = random_snappy(int(name[12:]))
        else:
            _cache[name] = NAMED[name]()
        for p in _cache[name]:
            assert len(p.ref) <= 1 << 20
    return _cache[name]


CASE_NAMES = (list(NAMED) + ["mixed_arena"]
              + [f"rand_lz4_{s}" for s in RANDOM_SEEDS]
              + [f"rand_snappy_{s}" for s in RANDOM_SEEDS])
MODES = ("auto", "segment", "litpar", "fallback")


# --------------------------------------------------------------------
# running a case and checking an arena
# --------------------------------------------------------------------
def run_case(pages, mode="auto", raw_lead=0, host=None, session=None,
             sentinel=0xA5):
    from parseable_amd import _lib

    return _lib.decompress_pages(
        [(p.codec, p.comp, len(p.ref)) for p in pages], mode=mode,
        raw_lead=raw_lead, host=host, session=session, sentinel=sentinel)


def image_offsets(pages) -> list:
    offs, o = [], 0
    for p in pages:
        offs.append(o)
        o += (len(p.ref) + 15) & ~15
    return offs + [o]


def expected_arena(pages, guard_len: int, sentinel: int = 0xA5) -> bytes:
    offs = image_offsets(pages)
    want = bytearray([sentinel]) * (offs[-1] + guard_len)
    for p, o in zip(pages, offs):
        want[o:o + len(p.ref)] = p.ref
    return bytes(want)


def _record_kind(page: Page, st: dict, rel: int) -> str:
    """which record kind writes image byte `rel` of a page on path st['mode']"""
    mode = st["mode"]
    if mode in ("raw", "host_image"):
        return {"raw": "raw segment copy (k_lz4_seg)",
                "host_image": "host-staged image"}[mode]
    if page.codec == "snappy":
        spans = _snappy_spans(page.comp)
    else:
        spans = _lz4_spans(page.comp)
    for i, (kind, dst, ln, off) in enumerate(spans):
        if dst <= rel < dst + ln:
            where = f"element {i}: {kind} dst={dst} len={ln}" + (
                f" off={off}" if kind == "match" else "")
            if mode == "litpar":
                k = (("k_lit_lane" if ln <= 256 else "k_lit_wave")
                     if kind == "literal" else
                     ("k_brres_inl / k_brres_lane" if ln <= 256 else "k_brres_wave"))
            elif kind == "literal":
                k = "k_lz4_seg literal copy"
            elif mode == "fallback":
                k = ("k_lz4_seg in-segment match, or k_lz4_backrefs "
                     + ("far" if off + ln > BR_FAR else "window") + " record")
            else:
                k = ("k_lz4_seg in-segment match, or deferred "
                     + ("k_brres_lane" if ln <= 256 else "k_brres_wave") + " record")
            return f"{k} ({where})"
    return "no element covers it"


def _lz4_spans(block: bytes):
    s, d, n = 0, 0, len(block)
    while s < n:
        token = block[s]; s += 1
        lit = token >> 4
        if lit == 15:
            while True:
                b = block[s]; s += 1; lit += b
                if b != 255:
                    break
        if lit:
            yield ("literal", d, lit, 0)
        s += lit; d += lit
        if s >= n:
            break
        off = block[s] | (block[s + 1] << 8); s += 2
        ml = token & 15
        if ml == 15:
            while True:
                b = block[s]; s += 1; ml += b
                if b != 255:
                    break
        ml += 4
        yield ("match", d, ml, off)
        d += ml


def _snappy_spans(block: bytes):
    s = 0
    while block[s] & 0x80:
        s += 1
    s += 1
    d, n = 0, len(block)
    while s < n:
        tag = block[s]; s += 1
        kind = tag & 3
        if kind == 0:
            ln = (tag >> 2) + 1
            if ln > 60:
                extra = ln - 60
                ln = int.from_bytes(block[s:s + extra], "little") + 1
                s += extra
            yield ("literal", d, ln, 0)
            s += ln; d += ln
        else:
            if kind == 1:
                ml = ((tag >> 2) & 7) + 4
                off = ((tag >> 5) << 8) | block[s]; s += 1
            else:
                nb = 2 if kind == 2 else 4
                ml = (tag >> 2) + 1
                off = int.from_bytes(block[s:s + nb], "little"); s += nb
            yield ("match", d, ml, off)
            d += ml


def check_arena(label: str, pages, arena: bytes, stats, guard_len: int,
                sentinel: int = 0xA5) -> None:
    """images equal the references byte for byte and every sentinel byte
    outside them (padding between images, trailing guard) is untouched; the
    failure names the first differing offset and what should have written it"""
    want = expected_arena(pages, guard_len, sentinel)
    assert len(arena) == len(want), f"{label}: arena {len(arena)} != {len(want)}"
    if arena == want:
        return
    first = next(i for i in range(len(want)) if arena[i] != want[i])
    offs = image_offsets(pages)
    where = "trailing guard"
    for pi, p in enumerate(pages):
        if offs[pi] <= first < offs[pi + 1]:
            rel = first - offs[pi]
            if rel >= len(p.ref):
                where = f"padding after page {pi} ({p.codec}, path {stats[pi]['mode']})"
            else:
                where = (f"page {pi} ({p.codec}, {len(p.ref)} bytes, path "
                         f"{stats[pi]['mode']}) offset {rel}: "
                         + _record_kind(p, stats[pi], rel))
            break
    n_bad = sum(1 for a, b in zip(arena, want) if a != b)
    raise AssertionError(
        f"{label}: first difference at arena offset {first} "
        f"(got {arena[first]:#04x}, want {want[first]:#04x}; {n_bad} bytes differ) "
        f"in {where}")
