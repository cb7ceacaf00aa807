"""CPU: bench.py's ``--dump-outputs`` writer -- float64 files, the size bound, the same seeded sample on every run."""
import numpy as np

import bench


def _dump(path, limit):
    rng = np.random.default_rng(3)
    arrays = {"comps": (rng.normal(size=(8, 5000, 3)), 1), "weigs": (rng.normal(size=(40, 8)), 0),
              "selected_vertices": (np.arange(8, dtype=np.int64) * 7, 0)}
    bench.dump_outputs(str(path), arrays, limit=limit)
    return arrays, {p.stem: np.load(p) for p in path.glob("*.npy")}, sum(p.stat().st_size for p in path.glob("*.npy"))


def test_small_outputs_are_written_whole(tmp_path):
    arrays, out, _ = _dump(tmp_path, limit=10 ** 7)
    assert sorted(out) == ["comps", "selected_vertices", "weigs"]
    for name, (a, _) in arrays.items():
        assert out[name].dtype == np.float64 and np.array_equal(out[name], a)


def test_large_outputs_are_a_seeded_sample_within_the_limit(tmp_path):
    arrays, out, nbytes = _dump(tmp_path / "a", limit=3 * 10 ** 5)
    assert nbytes <= 3 * 10 ** 5
    rows = out["comps_sample"].astype(np.int64)
    assert 0 < rows.size < 5000 and np.all(np.diff(rows) > 0)
    assert np.array_equal(out["comps"], arrays["comps"][0][:, rows])
    assert np.array_equal(out["weigs"], arrays["weigs"][0])             # under its share: whole
    _, again, _ = _dump(tmp_path / "b", limit=3 * 10 ** 5)
    assert all(np.array_equal(out[k], again[k]) for k in out)
