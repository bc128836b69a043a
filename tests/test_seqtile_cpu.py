"""Litpar sequence tiles without a GPU: the planner's records replayed
serially on the host (gpuq_test_decompress, host modes) over the cases of
tests/seqtile_common.py. The kernel itself is tests/test_gpu_seqtile.py."""

import subprocess

import pytest

from tests import decomp_common as dc
from tests import seqtile_common as sc
from tests.conftest import REPO_ROOT


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.run(["make", "-C", f"{REPO_ROOT}/parseable_amd/csrc"],
                   check=True, capture_output=True)


def test_tile_model_rule():
    m = sc.TileModel()
    m.lit(3); m.match(8, 5)            # one merged record
    m.match(8, 5)                      # literal-less record
    m.lit(4); m.lit(5)                 # match-less record, then a pending one
    m.match(9, 12)                     # not inlinable: flushes, closes
    m.lit(257); m.match(1, 256)        # long literal closes; record alone
    m.end()
    assert (m.n_tile, m.n_tile_rec) == (2, 5)


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_host_replay_of_tiles_matches_reference(name):
    tiled = sc.case(name)
    pages = [t.page for t in tiled]
    arena, st, guard, err = dc.run_case(pages, "litpar", host="decode")
    assert err == 0
    dc.check_arena(f"{name}/host-decode", pages, arena, st, guard)
    for lead in sc.leads(name):
        arena, st, guard, _ = dc.run_case(pages, "litpar", raw_lead=lead,
                                          host="replay", sentinel=0x3C)
        assert arena == dc.expected_arena(pages, guard, sentinel=0x3C), \
            f"{name}/lead{lead}/replay"
        for i, (t, s) in enumerate(zip(tiled, st)):
            assert s["mode"] == "litpar", f"{name} page {i}: {s}"
            assert (s["n_tile"], s["n_tile_rec"]) == (t.n_tile, t.n_tile_rec), \
                f"{name} page {i}: {s}"


def test_stated_counts():
    assert [t.n_tile for t in sc.case("count_edges")] == [1, 1, 2, 2, 3]
    assert [t.n_tile_rec for t in sc.case("count_edges")] == [255, 256, 257, 512, 513]
    # breakers: each kind took its own path next to the tiles
    for ki, kind in enumerate(sc.BREAKERS):
        pages = [t.page for t in sc.case("breakers")[3 * ki:3 * ki + 3]]
        for s in dc.run_case(pages, "litpar", host="decode")[1]:
            assert s["n_lit_wave"] == (kind == "lit257")
            assert s["n_res_lane"] == (kind == "period9")
            assert s["n_res_wave"] == (kind == "match257")
    # records that carry only one part exist where the case says so
    a, b = dc.run_case([t.page for t in sc.case("snappy_runs")], "litpar",
                       host="decode")[1]
    assert a["n_tile_rec"] > max(a["n_lit_lane"], a["n_inl"])
    assert b["n_tile_rec"] == b["n_inl"] == 300 and b["n_lit_lane"] == 1
