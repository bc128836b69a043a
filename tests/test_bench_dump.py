"""bench.py --dump-outputs: the result table of the timed path is written
column by column as float arrays that two builds can be compared on."""

import numpy as np

import bench


def test_dump_outputs_columns(tmp_path):
    query = {
        "select": [{"agg": "count_star"}, {"agg": "max", "col": "latency"},
                   {"agg": "avg", "col": "f_f64"}],
        "group_by": ["host", {"bin": "p_timestamp", "stride_ms": 60_000,
                              "origin": 0}],
    }
    rows = [
        ["host-0001", 60_000, 7, 999_999, 0.25],
        ["host-02", 120_000, 2**40, None, 1.5],
        [None, 0, 0, -3, None],
    ]
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), rows, query)
    assert sorted(p.name for p in out.iterdir()) == [
        "agg0_count_star.npy", "agg1_max_latency.npy", "agg2_avg_f_f64.npy",
        "key0_host.npy", "key1_bin_p_timestamp.npy"]

    host = np.load(out / "key0_host.npy")
    assert host.dtype == np.float32 and host.shape == (3, 9)
    assert bytes(host[0].astype(np.uint8)) == b"host-0001"
    assert bytes(host[1].astype(np.uint8)) == b"host-02\0\0"
    assert (host[2] == -1).all()

    for name, want in [
        ("key1_bin_p_timestamp", [60_000, 120_000, 0]),
        ("agg0_count_star", [7, 2**40, 0]),
        ("agg1_max_latency", [999_999, np.nan, -3]),
        ("agg2_avg_f_f64", [0.25, 1.5, np.nan]),
    ]:
        got = np.load(out / f"{name}.npy")
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, np.array(want, dtype=np.float64))


def test_dump_outputs_no_group_by(tmp_path):
    query = {"select": [{"agg": "count_star"}]}
    bench.dump_outputs(str(tmp_path), [[123]], query)
    np.testing.assert_array_equal(
        np.load(tmp_path / "agg0_count_star.npy"), np.array([123.0]))
