"""bench.py --dump-outputs on the host side: fields that fit are written whole, a field beyond the budget becomes a sample at
seeded positions that are the same from run to run, and everything is float64 within the budget."""
import numpy as np

import bench


def _dump(tmp_path, monkeypatch, budget, large, small):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", budget)
    bench.dump_outputs(str(tmp_path), large, small)
    return {p.stem: np.load(p) for p in tmp_path.glob("*.npy")}


def test_fields_within_the_budget_are_written_whole(tmp_path, monkeypatch):
    u, psi = np.arange(1000.0), -np.arange(500.0)
    d = _dump(tmp_path, monkeypatch, 64_000, {"u": u, "psi": psi}, {"history": np.ones((3, 8))})
    assert set(d) == {"u", "psi", "history"}
    assert np.array_equal(d["u"], u) and np.array_equal(d["psi"], psi) and d["history"].shape == (3, 8)
    assert all(a.dtype == np.float64 for a in d.values())


def test_a_field_beyond_the_budget_is_a_seeded_sample(tmp_path, monkeypatch):
    rng = np.random.default_rng(1)
    u, psi = rng.random(4000), rng.random(6000)
    budget = 8 * 4000 + 16 * 1000
    d = _dump(tmp_path / "a", monkeypatch, budget, {"u": u, "psi": psi}, {})
    assert np.array_equal(d["u"], u)
    idx = d["psi_index"].astype(np.int64)
    assert len(idx) == 1000 and np.all(np.diff(idx) > 0) and idx[-1] < len(psi)
    assert np.array_equal(d["psi"], psi[idx])
    assert sum(a.nbytes for a in d.values()) <= budget
    d2 = _dump(tmp_path / "b", monkeypatch, budget, {"u": u, "psi": psi}, {})  # same arguments, same positions
    assert np.array_equal(d2["psi_index"], d["psi_index"])


def test_the_headline_mesh_fits_in_64_mb(tmp_path):
    n = 2049 * 2049  # 2048^2 P1: u and psi, one value per vertex each
    bench.dump_outputs(str(tmp_path), {"u": np.zeros(n), "psi": np.zeros(n)}, {"history": np.zeros((500, 8))})
    assert sum(p.stat().st_size for p in tmp_path.glob("*.npy")) <= 64_000_000
    assert np.load(tmp_path / "u.npy").size == n
