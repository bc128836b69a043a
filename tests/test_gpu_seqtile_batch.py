"""k_seq_tile<K>: K sequence tiles per block (GPUQ_SEQ_TILE_BATCH = 1, 2, 4,
8 and unset) against the byte-loop reference decoders, in forced litpar mode.

Every run below is one gpuq_test_decompress call over several pages, so its
tiles form one tile array and a block's batch spans pages: non-contiguous
dst0, a different dst0 & 15 per tile, a partial last batch. For each K the
images equal the references byte for byte, every sentinel byte outside them
is untouched, the error word is 0 and the arena is the one every other K
produced. Pages are built and reference-decoded once per process."""

import pytest

from tests import decomp_common as dc
from tests import seqtile_common as sc

pytestmark = pytest.mark.gpu

BATCHES = (None, "1", "2", "4", "8")
LEADS = (0, 1, 7, 15)


@pytest.fixture(scope="module")
def session():
    from parseable_amd import GpuSession

    sess = GpuSession()
    yield sess._ctx
    sess.close()


# --------------------------------------------------------------------
# pages
# --------------------------------------------------------------------
def _recs_page(n: int, seed: int, shift: int = 0) -> sc.Tiled:
    """n eligible records (the final literal is the last): 8-byte PLAIN-shaped
    records behind a first record of 16 + shift bytes, so the page's second
    tile starts at shift (mod 8) and not on a 16 B boundary"""
    t = sc.Lz4Tiles(seed)
    t.seq(t.b.rand(3 + shift) + bytes(5) + t.b.rand(3), 8, 5).plain(n - 2)
    x = t.done()
    assert (x.n_tile, x.n_tile_rec) == ((n + 255) // 256, n)
    return x


def _small(seed: int, n: int = 20) -> sc.Tiled:
    x = _recs_page(n, seed, shift=seed % 8)
    assert x.n_tile == 1
    return x


def _full_tile_page(seed: int) -> sc.Tiled:
    """32 records of 512 bytes = one full 16384-byte tile, then the final
    literal alone in a 1-record tile"""
    t = sc.Lz4Tiles(seed)
    for _ in range(32):
        t.seq(256, 1 + t.b.d % 8, 256)
    x = t.done()
    assert t.m.closed_at == [16384] and (x.n_tile, x.n_tile_rec) == (2, 33)
    return x


def _stage_edge_page(seed: int, tail: int) -> sc.Tiled:
    """a full 16384-byte tile at dst0 & 15 == 1 and a 1-record tile of `tail`
    bytes behind it, also at 1 (mod 16). Packed, the pair takes 16400 +
    align16(1 + tail) bytes of stage: with tail = 15 that is the 16416 bytes
    of the K = 2 stage exactly, with tail = 16 it is 16 over."""
    t = sc.Lz4Tiles(seed)
    t.seq(257, 8, 5)                    # k_lit_wave, then a literal-less record
    t.seq(251, 3, 256)                  # 5 + 507 = 512
    for _ in range(31):
        t.seq(256, 1 + t.b.d % 8, 256)
    x = t.done(tail=tail)
    assert t.m.closed_at == [16384] and (x.n_tile, x.n_tile_rec) == (2, 34)
    return x


def _edge_records_page() -> sc.Tiled:
    """match-only records of every period 1..8, literals of 255 / 256 bytes
    with and without a match, literal lengths around the 8-byte load"""
    t = sc.Lz4Tiles(8300).seq(11, 8, 5)
    for p in range(1, 9):
        t.seq(0, p, 4 + p).seq(0, p, 256)
    for n in (1, 7, 8, 9, 15, 16, 17, 255, 256):
        t.seq(n, 1 + n % 8, 4 + n % 5)
    t.seq(256, 8, 256).seq(0, 1, 4)
    x = t.done(tail=16)
    assert x.n_tile == 1
    return x


def _snappy_literal_only() -> sc.Tiled:
    """snappy: literal-only records back to back (a 256-byte one among them),
    then copy-only records"""
    t = sc.SnappyTiles(8301).lit(8).lit(5).lit(256, 2).lit(7).lit(1)
    for p in range(1, 9):
        t.copy(p, 3 + p)
    t.lit(60).copy(8, 11)
    x = t.done()
    assert x.n_tile == 1
    return x


def _end_page() -> sc.Tiled:
    """a page whose length is a multiple of 16: the last tile's flush ends
    where the trailing guard begins"""
    t = sc.Lz4Tiles(8302).first_value().plain(300)
    x = t.done(tail=12 + (-(t.b.d + 12)) % 16)
    assert len(x.page.ref) % 16 == 0 and x.n_tile == 2
    return x


# tile totals 1, K-1, K, K+1 and 2K+1 for K = 2, 4, 8, from pages of 255,
# 256, 257, 512 and 513 records
COUNT_RUNS = {
    1: (255,),
    2: (257,),
    3: (513,),
    4: (256, 513),
    5: (257, 513),
    7: (512, 513, 257),
    8: (513, 513, 512),
    9: (255, 513, 513, 257),
    17: (513, 513, 513, 513, 513, 257),
}


def _count_run(total: int) -> list:
    pages = [_recs_page(n, 8000 + 10 * total + i, shift=(3 * i + total) % 8)
             for i, n in enumerate(COUNT_RUNS[total])]
    assert sum(p.n_tile for p in pages) == total
    return pages


def _stage_fit() -> list:
    """full tiles at tile indices 0, 11, 15 and 21 of the run: first, middle
    and last slot of a batch for K = 4 and 8, both slots for K = 2"""
    s = iter(range(8100, 8200))
    run = [_full_tile_page(next(s))]                          # tiles 0, 1
    run += [_small(next(s)) for _ in range(9)]                # 2..10
    run += [_full_tile_page(next(s))]                         # 11, 12
    run += [_small(next(s)) for _ in range(2)]                # 13, 14
    run += [_full_tile_page(next(s))]                         # 15, 16
    run += [_small(next(s)) for _ in range(4)]                # 17..20
    run += [_full_tile_page(next(s))]                         # 21, 22
    full_at, idx = [], 0
    for p in run:
        if p.n_tile == 2:
            full_at.append(idx)
        idx += p.n_tile
    assert full_at == [0, 11, 15, 21]
    return run


def _mixed() -> list:
    """1-record tiles beside 256-record tiles, the record edges, both codecs
    in one run, the last flush against the guard"""
    return [_edge_records_page(), _recs_page(257, 8310, shift=5),
            _snappy_literal_only(), _recs_page(256, 8311, shift=1),
            sc.case("snappy_runs")[1], _recs_page(513, 8312, shift=7),
            _end_page()]


RUNS = {f"tiles{n}": (lambda n=n: _count_run(n)) for n in COUNT_RUNS}
RUNS["stage_fit"] = _stage_fit
RUNS["stage_exact"] = lambda: [_stage_edge_page(8201, 15), _small(8202)]
RUNS["stage_over"] = lambda: [_stage_edge_page(8203, 16), _small(8204)]
RUNS["mixed"] = _mixed

_cache: dict = {}


def _run(name: str) -> list:
    if name not in _cache:
        _cache[name] = RUNS[name]()
    return _cache[name]


def _leads(name: str) -> tuple:
    return LEADS if name.startswith("tiles") else (0, 7)


@pytest.mark.parametrize("name", list(RUNS))
def test_gpu_batched_tiles_match_reference(session, monkeypatch, name):
    tiled = _run(name)
    pages = [t.page for t in tiled]
    host_stats = dc.run_case(pages, "litpar", host="decode")[1]
    for lead in _leads(name):
        sentinel = 0xA5 if lead != 1 else 0x00
        arenas = {}
        for k in BATCHES:
            if k is None:
                monkeypatch.delenv("GPUQ_SEQ_TILE_BATCH", raising=False)
            else:
                monkeypatch.setenv("GPUQ_SEQ_TILE_BATCH", k)
            label = f"{name}/litpar/lead{lead}/batch{k}"
            try:
                arena, st, guard, d_err = dc.run_case(
                    pages, "litpar", raw_lead=lead, session=session,
                    sentinel=sentinel)
            except RuntimeError as e:
                if "HIP error" in str(e):
                    # a device fault: launch nothing more onto this GPU
                    pytest.exit(f"{label}: {e}", returncode=3)
                raise
            assert d_err == 0, f"{label}: d_err {d_err}"
            assert st == host_stats, f"{label}: stats differ from host-only mode"
            assert [(s["n_tile"], s["n_tile_rec"]) for s in st] == \
                [(t.n_tile, t.n_tile_rec) for t in tiled]
            dc.check_arena(label, pages, arena, st, guard, sentinel=sentinel)
            arenas[k] = arena
        assert all(a == arenas["1"] for a in arenas.values()), \
            f"{name}/lead{lead}: arenas differ between batch sizes"
