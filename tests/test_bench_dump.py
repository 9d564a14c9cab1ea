"""bench.py --dump-outputs (CPU): the files, their dtype and shapes, and the fixed seeded sample
taken of an output past the size caps."""
import numpy as np

import bench


def _dump(tmp_path, name, n_shares, n_cts):
    rng = np.random.default_rng(7)
    st = rng.integers(0, 3, n_shares).astype(np.int32)
    g = rng.integers(0, 256, 48 * n_cts).astype(np.uint8)
    cst = rng.integers(0, 2, n_cts).astype(np.int32)
    d = tmp_path / name
    bench.dump_outputs(str(d), st, g, cst)
    return st, g, cst, {p.name: np.load(p) for p in d.iterdir()}


def test_dump_outputs_whole(tmp_path):
    st, g, cst, got = _dump(tmp_path, "a", 1000, 10)
    assert sorted(got) == ["combine_status.npy", "combined_g1.npy", "status.npy"]
    assert all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got["status.npy"], st)
    assert np.array_equal(got["combined_g1.npy"], g.reshape(10, 48))
    assert np.array_equal(got["combine_status.npy"], cst)


def test_dump_outputs_sample_is_fixed(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_SHARES", 100)
    monkeypatch.setattr(bench, "DUMP_MAX_CTS", 4)
    st, g, cst, a = _dump(tmp_path, "a", 1000, 10)
    _, _, _, b = _dump(tmp_path, "b", 1000, 10)
    assert a["status.npy"].shape == (100,) and a["combined_g1.npy"].shape == (4, 48)
    assert a["combine_status.npy"].shape == (4,)
    for k in a:
        assert np.array_equal(a[k], b[k])
    # rows of the output, in order: the points and the combine statuses of the same ciphertexts
    rows = [int(np.flatnonzero((g.reshape(10, 48) == r).all(axis=1))[0]) for r in a["combined_g1.npy"]]
    assert rows == sorted(rows) and np.array_equal(a["combine_status.npy"], cst[rows])
