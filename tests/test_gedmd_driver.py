"""The drivers' optional `gedmd` key inside config.observables: not handed to the integrator, completed and validated, the weights
formed as the reference's calculate_weights forms them, and three arrays written next to today's (the GPU call is replaced by a
stand-in here; tests/test_gpu_gedmd.py runs the real one)."""
import types

import numpy as np
import pytest

from conftest import pkg


def test_gedmd_key_parsing():
    ti = pkg()
    dr = ti.drivers
    cfg = types.SimpleNamespace(observables={"descriptors": [["coord", 0]], "every": 2, "gedmd": {"p": 24}})
    assert dr._observe_kw(cfg)["observe"] == {"descriptors": [["coord", 0]], "every": 2}
    assert dr._gedmd_settings({"descriptors": []}) is None
    g = dr._gedmd_settings(cfg.observables)
    assert g == {"p": 24, "sigma": 0.6, "nev": 4, "tol": 1e-4, "n_boot": 1000, "seed": 0, "potential": (4.0, 0.5)}
    g = dr._gedmd_settings({"gedmd": {"p": 8, "sigma": 1.5, "nev": 2, "tol": 0.0, "n_boot": 10, "seed": 3, "potential": [1, 0]}})
    assert g == {"p": 8, "sigma": 1.5, "nev": 2, "tol": 0.0, "n_boot": 10, "seed": 3, "potential": (1.0, 0.0)}
    for bad in (5, {"q": 1}, {"p": 0}, {"p": 2.5}, {"nev": True}, {"n_boot": 0}, {"seed": -1}, {"sigma": 0.0}, {"sigma": float("nan")}, {"tol": -1.0},
                {"potential": [1.0]}, {"potential": [1.0, float("inf")]}, {"p": 3, "nev": 4}):
        with pytest.raises(ValueError, match="gedmd"):
            dr._gedmd_settings({"gedmd": bad})


def test_gedmd_key_adds_three_arrays_and_nothing_else(tmp_path, monkeypatch):
    ti = pkg()
    obs, dr = ti.observables, ti.drivers
    cfg = types.SimpleNamespace(observables={"descriptors": [["coord", 0]], "bins": 4, "gedmd": {"p": 6, "nev": 2, "n_boot": 5, "seed": 9, "potential": [2.0, 0.25]}})
    seen = {}

    def fake_summary(cv, dl, bins=32, engine=None):
        return np.zeros((cv.shape[1], bins)), np.zeros((cv.shape[1], bins + 1)), 3.5

    def fake_generator(values, omega, nev, a, **kw):
        seen.update(values=np.asarray(values), omega=omega, nev=nev, a=a, kw=kw)
        return obs.GedmdResult(np.array([-2.0, 0.0]), np.array([[-2.5, -0.1], [-1.5, 0.1]]), np.zeros((5, 2)), np.zeros((6, 2)), 4)

    monkeypatch.setattr(obs, "end_state_summary", fake_summary)
    monkeypatch.setattr(obs, "gedmd_generator", fake_generator)
    cvs = [np.zeros((3, 4, 1), np.float32), np.zeros((3, 2, 1), np.float32)]
    dlogps = [np.array([0.5, 1.0, -1.0, 2.0], np.float32), np.array([0.25, 0.0], np.float32)]
    x0 = np.array([-1.0, 1.0, 0.5, -0.5, 1.5, 0.0])
    x1 = np.array([-0.9, 1.1, 0.25, -1.25, 1.0, 0.125])
    dr._write_observables(cfg, str(tmp_path / "with.npz"), cvs, dlogps, gedmd=(x0, x1, 1.0, 1.25))
    z = np.load(tmp_path / "with.npz")
    assert sorted(z.files) == ["cv", "edges", "ess", "gedmd_ci", "gedmd_eigenvalues", "gedmd_rank", "hist"]
    np.testing.assert_array_equal(z["gedmd_eigenvalues"], [-2.0, 0.0])
    np.testing.assert_array_equal(z["gedmd_ci"], [[-2.5, -0.1], [-1.5, 0.1]])
    assert int(z["gedmd_rank"]) == 4
    U = lambda x: 2.0 * (x * x - 1.0) ** 2 + 0.25 * x
    logw = (1.0 * U(x0) - 1.25 * U(x1) - np.concatenate(dlogps).astype(np.float64)).astype(np.float32)
    np.testing.assert_array_equal(seen["kw"]["logw"], logw)
    assert seen["kw"]["logw"].dtype == np.float32 and seen["values"].dtype == np.float32
    np.testing.assert_array_equal(seen["values"], x1.astype(np.float32))
    np.testing.assert_array_equal(seen["omega"], np.random.RandomState(9).randn(1, 6) / 0.6)
    assert seen["nev"] == 2 and seen["a"] == 2.0 / 1.25 and seen["kw"]["n_boot"] == 5 and seen["kw"]["seed"] == 9 and seen["kw"]["tol"] == 1e-4
    # the weights need dlogp and the adw driver's samples
    with pytest.raises(ValueError, match="return_dlogp"):
        dr._write_observables(cfg, str(tmp_path / "bad.npz"), cvs, [], gedmd=(x0, x1, 1.0, 1.25))
    with pytest.raises(ValueError, match="sample_adw"):
        dr._write_observables(cfg, str(tmp_path / "bad.npz"), cvs, dlogps)
    # without the key: today's arrays in today's order, and no call
    del cfg.observables["gedmd"]
    seen.clear()
    dr._write_observables(cfg, str(tmp_path / "without.npz"), cvs, dlogps, gedmd=(x0, x1, 1.0, 1.25))
    z0 = np.load(tmp_path / "without.npz")
    assert z0.files == ["cv", "hist", "edges", "ess"] and not seen
