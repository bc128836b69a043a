"""The dictionary run-header scan fixtures (tests/dictwalk_common.py) hold
the run structure they are named for: checked on the written files with the
page walk of dw.idx_pages (pc's Thrift reader and hybrid decoder; pyarrow
only decompresses). No GPU.

What the scan of dict_page_decode relies on, and what is pinned here:
  - a bit-packed run closes at 63 groups: header byte 0x7F, 504 values;
  - an RLE run starts where 8 equal values fill a group, and its header
    takes 1, 2 or 3 bytes for counts below 64, below 8192, and above;
  - the decoy page has data bytes equal to the header the scan expects at
    offsets it probes after a mismatch.
A one-entry dictionary is written with index width 1 by this writer, not 0:
width 0 with values present cannot be produced here (test_one_entry pins
that, so a writer that starts emitting width 0 shows up).
"""

import pytest

from tests import dictwalk_common as dw

FULL = (dw.GROUPS << 1) | 1       # 0x7F


@pytest.fixture(scope="module")
def fs(tmp_path_factory):
    return dw.FixtureSet(tmp_path_factory.mktemp("dictwalk_cpu"))


def _page(fs, name, nul=False, col="s"):
    names = list(fs.shapes)
    case = fs.cases(nul)[names.index(name)]
    pages = dw.idx_pages(case.path, col)
    assert len(pages) == 1, f"{name}: {len(pages)} pages"
    assert pages[0]["idx"] is not None
    return pages[0]


def _kinds(page):
    return [(k, n) for k, _, n in page["runs"]]


def _same_partition(idx, want):
    """idx equals want up to a renaming of the indices (the writer numbers
    dictionary entries by first appearance)."""
    fwd = {}
    for a, b in zip(idx, want):
        if fwd.setdefault(b, a) != a:
            return False
    return len(idx) == len(want) and len(set(fwd.values())) == len(fwd)


@pytest.mark.parametrize("nul", [False, True], ids=["nn", "nul"])
@pytest.mark.parametrize("n", dw.PURE_N)
def test_pure_pages(fs, n, nul):
    """Only bit-packed runs: full 504-value runs, then one clipped run (an
    RLE run of one where a single value is left over)."""
    pg = _page(fs, f"pure_{n}", nul)
    assert pg["n"] == n and _same_partition(pg["idx"], fs.shapes[f"pure_{n}"])
    want = [("packed", dw.RUN)] * (n // dw.RUN)
    if n % dw.RUN:
        want.append(("packed", n % dw.RUN))
    if n % dw.RUN == 1:     # a lone last value closes as an RLE run of one
        want[-1] = ("rle", 1)
    assert _kinds(pg) == want
    hd = dw.headers(pg)
    assert all(h == FULL and nb == 1 for _, h, nb in hd[:n // dw.RUN])
    # equal headers at a fixed stride: what one scan step accepts
    offs = [o for o, _, _ in hd[:n // dw.RUN]]
    assert offs == [k * (1 + dw.GROUPS * pg["bw"]) for k in range(len(offs))]


@pytest.mark.parametrize("nul", [False, True], ids=["nn", "nul"])
@pytest.mark.parametrize("c", dw.RLE_COUNTS)
@pytest.mark.parametrize("pos", dw.RLE_POS)
def test_one_rle_run(fs, pos, c, nul):
    """Exactly one RLE run, of count c, at run index pos; every run before
    it is a full bit-packed run; its header has the length c needs."""
    name = f"rle_{pos}_{c}"
    pg = _page(fs, name, nul)
    assert _same_partition(pg["idx"], fs.shapes[name])
    kinds = _kinds(pg)
    at = dw.STEP + 2 if pos == "last" else pos
    assert kinds[:at] == [("packed", dw.RUN)] * at
    assert kinds[at] == ("rle", c)
    assert [k for k, _ in kinds].count("rle") == 1
    assert (len(kinds) == at + 1) == (pos == "last")
    _, hdr, nbytes = dw.headers(pg)[at]
    assert hdr == c << 1
    assert nbytes == (1 if c < 64 else 2 if c < 8192 else 3)


def test_cut_short(fs):
    """A 10-group run cut by an RLE run, then full runs: the group count
    changes mid-page."""
    kinds = _kinds(_page(fs, "cut"))
    assert kinds[:2] == [("packed", 80), ("rle", 20)]
    assert kinds[2:7] == [("packed", dw.RUN)] * 5 and kinds[7] == ("packed", 3)


def test_alternating(fs):
    """2-group runs and RLE runs of 9 in turn: every scan step mismatches."""
    assert _kinds(_page(fs, "alt")) == [("packed", 16), ("rle", 9)] * 200


@pytest.mark.parametrize("bw", list(dw.WIDTHS))
def test_widths(fs, bw):
    pg = _page(fs, f"bw{bw}")
    assert pg["bw"] == bw
    kinds = _kinds(pg)
    assert len(kinds) >= dw.STEP + 2
    assert all(k == ("packed", dw.RUN) for k in kinds[:-1])
    x = _page(fs, f"bw{bw}", col="x")
    assert x["bw"] == bw and _kinds(x) == kinds


def test_big_width(fs):
    pg = dw.idx_pages(fs.big()[0].path, "x")
    assert len(pg) == 1 and pg[0]["bw"] == dw.BIG_WIDTH
    assert len(pg[0]["runs"]) >= dw.STEP + 2


def test_one_entry(fs):
    pg = _page(fs, "one")
    assert pg["bw"] == 1 and _kinds(pg) == [("rle", 100)]


@pytest.mark.parametrize("nul", [False, True], ids=["nn", "nul"])
def test_multipage(fs, nul):
    """Many small pages: MP_BATCH rows and at most two runs each, fewer
    runs than a block has waves; the _nul twin mixes all-valid pages (mode
    0) and null-bearing pages (mode 1) in one chunk."""
    from tests import pagecases_common as pc

    case = fs.cases(nul)[list(fs.shapes).index("mp")]
    pages = dw.idx_pages(case.path, "s")
    assert len(pages) >= dw.MP_PAGES
    assert sum(p["n"] for p in pages) == dw.MP_PAGES * pc.MP_BATCH
    assert all(len(p["runs"]) <= 2 for p in pages)
    if nul:     # all-valid and null-bearing pages in one chunk (modes 0, 1)
        rows = pc.inspect_file(case.path)["s"]["pages"]
        full = [all(n == 0 or k == "rle" for k, _, n in p["def_runs"])
                and len(p["def_runs"]) == 1 for p in rows]
        assert any(full) and not all(full)


def test_decoy(fs):
    """After the second RLE run breaks a scan step, the positions a stale
    stride probes lie in data bytes, and some of them hold 0x7F."""
    pg = _page(fs, "decoy")
    assert pg["bw"] == 8 and pg["idx"] == fs.shapes["decoy"]
    kinds = _kinds(pg)
    assert kinds[:6] == [("packed", 256), ("rle", 8)] + \
        [("packed", dw.RUN)] * 3 + [("rle", 8)]
    hd = dw.headers(pg)
    true_offsets = {o for o, _, _ in hd}
    stride = 1 + dw.GROUPS * 8
    # the scan parses run 2 serially, then probes from run 3 at this stride
    p0 = hd[3][0]
    probes = [p0 + k * stride for k in range(dw.STEP)
              if p0 + k * stride < len(pg["stream"])]
    assert pg["stream"][probes[0]] == FULL and pg["stream"][probes[1]] == FULL
    assert pg["stream"][probes[2]] == 8 << 1          # the RLE header
    stale = [o for o in probes[3:] if o not in true_offsets]
    assert stale and any(pg["stream"][o] == FULL for o in stale)
