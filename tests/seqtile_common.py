"""Cases for the litpar sequence tiles (k_seq_tile; tests/test_seqtile_cpu.py,
tests/test_gpu_seqtile.py). No GPU import.

Pages are built with the builders of tests/decomp_common.py (whose pyarrow
second opinion guards them) and run in forced `litpar` mode. Every page is
at most 64 KiB. Beside each page the builder states how many tiles and tile
records the planner must produce, by the rule of parseable_amd/csrc/
dev_types.h (DevSeq / DevSeqTile), modelled here from the stream alone:

- a literal run of <= 256 bytes and a match of <= 256 bytes whose pattern
  (min(offset, length) bytes) is <= 8 bytes are tile-eligible;
- an eligible literal and the eligible match right behind it are one record,
  any other eligible element a record of its own;
- a tile is a maximal run of records with contiguous output, closed at 256
  records, before the record that would take it past 16384 bytes, at any
  ineligible element and at the page end."""

from __future__ import annotations

from collections import namedtuple

from tests import decomp_common as dc

TILE_RECS = 256
TILE_BYTES = 16384

# a page and the tile / tile-record counts its plan must have
Tiled = namedtuple("Tiled", "page n_tile n_tile_rec")


class TileModel:
    def __init__(self):
        self.n_tile = self.n_tile_rec = 0
        self.open = False
        self.recs = self.out = 0
        self.pend = 0           # eligible literal waiting for its match
        self.closed_at = []     # out_len of every tile closed by the byte cap

    def _rec(self, n: int) -> None:
        if self.open and self.out + n > TILE_BYTES:
            self.closed_at.append(self.out)
            self.open = False
        if self.open and self.recs == TILE_RECS:
            self.open = False
        if not self.open:
            self.open, self.recs, self.out = True, 0, 0
            self.n_tile += 1
        self.recs += 1
        self.out += n
        self.n_tile_rec += 1

    def _flush(self) -> None:
        if self.pend:
            self._rec(self.pend)
            self.pend = 0

    def lit(self, n: int) -> None:
        self._flush()
        if n > 256:
            self.open = False
        else:
            self.pend = n

    def match(self, off: int, ml: int) -> None:
        if min(off, ml) <= 8 and ml <= 256:
            n, self.pend = self.pend + ml, 0
            self._rec(n)
        else:
            self._flush()
            self.open = False

    def end(self) -> None:
        self._flush()
        self.open = False


class Lz4Tiles:
    """Lz4Builder plus the tile model of what it builds"""

    def __init__(self, seed: int):
        self.b = dc.Lz4Builder(seed)
        self.m = TileModel()

    def seq(self, lit, off: int, ml: int) -> "Lz4Tiles":
        n = lit if isinstance(lit, int) else len(lit)
        if n:
            self.m.lit(n)
        self.m.match(off, ml)
        self.b.seq(lit, off, ml)
        return self

    def plain(self, n: int) -> "Lz4Tiles":
        """n sequences of the PLAIN int64 shape: 3 random literals, then the
        5 zero high bytes as a match at offset 8"""
        for _ in range(n):
            self.seq(3, 8, 5)
        return self

    def first_value(self) -> "Lz4Tiles":
        """the value the offset-8 matches start from, as one sequence"""
        return self.seq(self.b.rand(3) + bytes(5) + self.b.rand(3), 8, 5)

    def done(self, tail=12) -> Tiled:
        self.m.lit(tail)
        self.m.end()
        comp = self.b.finish(tail)
        assert self.b.d <= 65536
        return Tiled(dc.lz4_page(comp, self.b.d), self.m.n_tile, self.m.n_tile_rec)


class SnappyTiles:
    def __init__(self, seed: int):
        self.b = dc.SnappyBuilder(seed)
        self.m = TileModel()

    def lit(self, data, extra=None) -> "SnappyTiles":
        self.m.lit(data if isinstance(data, int) else len(data))
        self.b.lit(data, extra)
        return self

    def copy(self, off: int, ml: int, form=None) -> "SnappyTiles":
        self.m.match(off, ml)
        self.b.copy(off, ml, form)
        return self

    def done(self) -> Tiled:
        self.m.end()
        assert self.b.d <= 65536
        return Tiled(dc.snappy_page(self.b.finish()), self.m.n_tile,
                     self.m.n_tile_rec)


# --------------------------------------------------------------------
COUNT_EDGES = ((255, 1), (256, 1), (257, 2), (512, 2), (513, 3))


def count_edges() -> list:
    """pages of exactly n eligible records (the final literal is the last)"""
    out = []
    for n, tiles in COUNT_EDGES:
        t = Lz4Tiles(7000 + n).first_value().plain(n - 2).done()
        assert (t.n_tile, t.n_tile_rec) == (tiles, n)
        out.append(t)
    return out


def _big(t: Lz4Tiles, lit=256, ml=256) -> Lz4Tiles:
    """one record of lit + ml bytes, the match's period cycling 1..8"""
    return t.seq(lit, 1 + t.b.d % 8, ml)


def byte_cap() -> list:
    """512-byte records; the running out_len reaches 16383, 16384 and 16385
    at a record boundary, and the tile closes before the record that would
    pass 16384"""
    out = []
    # 511 + 31 * 512 = 16383: the 33rd record does not fit
    t = _big(Lz4Tiles(7101), lit=255)
    for _ in range(33):
        _big(t)
    assert t.m.closed_at == [16383]
    out.append(t.done())
    # 32 * 512 = 16384: full to the byte
    t = Lz4Tiles(7102)
    for _ in range(34):
        _big(t)
    assert t.m.closed_at == [16384]
    out.append(t.done())
    # 5 + 508 + 31 * 512 = 16385: the 33rd record itself would pass the cap
    t = _big(_big(Lz4Tiles(7103), lit=1, ml=4), lit=252)
    for _ in range(33):
        _big(t)
    assert t.m.closed_at == [16385 - 512]
    out.append(t.done())
    for x in out:
        assert x.n_tile == 2      # cap, then the rest up to the page end
    return out


def _breaker(t: Lz4Tiles, kind: str) -> None:
    if kind == "lit257":
        t.seq(257, 8, 5)          # k_lit_wave, then a literal-less record
    elif kind == "period9":
        t.seq(9, 9, 12)           # k_brres_lane
    else:
        t.seq(3, 1, 257)          # k_brres_wave


BREAKERS = ("lit257", "period9", "match257")


def breakers() -> list:
    out = []
    for ki, kind in enumerate(BREAKERS):
        for pi, pos in enumerate(("first", "middle", "last")):
            t = Lz4Tiles(7200 + 10 * ki + pi)
            if pos == "first":
                _breaker(t, kind)
                t.first_value().plain(40)
            elif pos == "middle":
                t.first_value().plain(20)
                _breaker(t, kind)
                t.plain(20)
            else:
                t.first_value().plain(40)
                _breaker(t, kind)
            # literal-less sequences back to back, then the final literal
            t.seq(0, 8, 5).seq(0, 3, 7).seq(0, 8, 256)
            out.append(t.done(tail=13 + pi))
    return out


ALIGN_LEADS = (0, 1, 7, 15)


def align() -> list:
    """a leading 257+k-byte literal (k_lit_wave) puts the first tile at every
    residue mod 16; literal lengths around 8 and 16 vary the raw reads"""
    out = []
    for k in range(16):
        t = Lz4Tiles(7300 + k).seq(257 + k, 8, 5).plain(12)
        for n in (7, 8, 9, 15, 16, 17, 31, 255, 256):
            t.seq(n, 1 + n % 8, 4 + n % 5)
        t.plain(9)
        x = t.done(tail=12 + k)
        assert x.n_tile == 1
        out.append(x)
    return out


def two_pages_tail() -> list:
    """page lengths of every residue 1..15 mod 16: the last tile of a page
    ends inside the inter-image padding's 16 bytes"""
    out = []
    for r in range(1, 16):
        t = Lz4Tiles(7400 + r).first_value().plain(30 + r)
        tail = 12 + (r - (t.b.d + 12)) % 16
        x = t.done(tail=tail)
        assert len(x.page.ref) % 16 == r
        out.append(x)
    return out


def snappy_runs() -> list:
    t = SnappyTiles(7500).lit(8)
    for _ in range(5):                      # copy-only runs: lit_len = 0
        t.copy(8, 5).copy(3, 7).copy(1, 64)
    t.lit(5).lit(7).copy(4, 9)              # two literals in a row
    t.lit(60).copy(8, 11).lit(61).copy(2, 33)   # 1-byte / 2-byte length form
    t.lit(60, 1).lit(61, 2).lit(256, 2).copy(7, 64)
    t.copy(20, 30)                          # not inlinable: closes the tile
    t.copy(5, 12).lit(3)
    t.lit(257).copy(6, 6).lit(1)
    a = t.done()
    assert a.n_tile == 3
    # more than one tile of copy-only records
    t = SnappyTiles(7501).lit(4)
    for i in range(300):
        t.copy(1 + i % 4, 1 + i % 64)
    b = t.done()
    assert (b.n_tile, b.n_tile_rec) == (2, 300)
    return [a, b]


NAMED = {
    "count_edges": count_edges,
    "byte_cap": byte_cap,
    "breakers": breakers,
    "align": align,
    "two_pages_tail": two_pages_tail,
    "snappy_runs": snappy_runs,
}
CASE_NAMES = tuple(NAMED)

_cache: dict = {}


def case(name: str) -> list:
    """[Tiled] of a case, built (and reference-decoded) once per process"""
    if name not in _cache:
        _cache[name] = NAMED[name]()
    return _cache[name]


def leads(name: str) -> tuple:
    return ALIGN_LEADS if name == "align" else (0, 5)
