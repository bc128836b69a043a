"""The page-decompression kernels against the byte-loop reference decoders.

gpuq_test_decompress runs plan build's page planning and execute's seven
decompress launches (k_lz4_seg, k_lit_lane, k_lit_wave, k_brres_inl,
k_brres_lane, k_brres_wave, k_lz4_backrefs) on the built streams of
tests/decomp_common.py. For every case, plan mode and source alignment:
the images equal the reference byte for byte, every sentinel byte outside
them is untouched, the kernels' error word is 0 and the path statistics
equal the host-only run's — whose path coverage tests/test_decomp_cpu.py
asserts, so a case cannot pass here without running the path it names."""

import pytest

from tests import decomp_common as dc

pytestmark = pytest.mark.gpu

RAW_LEADS = (0, 1, 15)


@pytest.fixture(scope="module")
def session():
    from parseable_amd import GpuSession

    sess = GpuSession()
    yield sess._ctx
    sess.close()


@pytest.mark.parametrize("mode", dc.MODES)
@pytest.mark.parametrize("name", dc.CASE_NAMES)
def test_gpu_decompress_matches_reference(session, name, mode):
    pages = dc.case(name)
    host_stats = dc.run_case(pages, mode, host="decode")[1]
    if mode == "litpar" and not any(s["mode"] == "litpar" and p.codec == "lz4_raw"
                                    for p, s in zip(pages, host_stats)):
        # the litpar walk refuses every LZ4 page of this case (or there is
        # none): the plan is the auto / segment one, tested under its name
        assert host_stats == dc.run_case(pages, "segment", host="decode")[1]
        return
    for lead in RAW_LEADS:
        sentinel = 0xA5 if lead != 1 else 0x00
        label = f"{name}/{mode}/lead{lead}"
        try:
            arena, st, guard, d_err = dc.run_case(
                pages, mode, raw_lead=lead, session=session, sentinel=sentinel)
        except RuntimeError as e:
            if "HIP error" in str(e):
                # a device fault: launch nothing more onto this GPU
                pytest.exit(f"{label}: {e}", returncode=3)
            raise
        assert d_err == 0, f"{label}: d_err {d_err}"
        assert st == host_stats, f"{label}: stats differ from host-only mode"
        dc.check_arena(label, pages, arena, st, guard, sentinel=sentinel)
