"""k_seq_tile against the byte-loop reference decoders, on the cases of
tests/seqtile_common.py in forced litpar mode: images equal the references
byte for byte, every sentinel byte outside them is untouched, the kernels'
error word is 0 and the plan is the one tests/test_seqtile_cpu.py checks."""

import pytest

from tests import decomp_common as dc
from tests import seqtile_common as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def session():
    from parseable_amd import GpuSession

    sess = GpuSession()
    yield sess._ctx
    sess.close()


@pytest.mark.parametrize("name", sc.CASE_NAMES)
def test_gpu_tiles_match_reference(session, name):
    tiled = sc.case(name)
    pages = [t.page for t in tiled]
    host_stats = dc.run_case(pages, "litpar", host="decode")[1]
    for lead in sc.leads(name):
        sentinel = 0xA5 if lead != 1 else 0x00
        label = f"{name}/litpar/lead{lead}"
        try:
            arena, st, guard, d_err = dc.run_case(
                pages, "litpar", raw_lead=lead, session=session, sentinel=sentinel)
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
