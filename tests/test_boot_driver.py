"""The drivers' optional `bootstrap` key inside config.observables: not handed to the integrator, validated, and written as ess_ci /
ess_boot next to today's arrays (the GPU call is replaced by a stand-in here; tests/test_gpu_boot.py runs the real one)."""
import types

import numpy as np
import pytest

from conftest import pkg


def test_bootstrap_key_adds_two_arrays_and_nothing_else(tmp_path, monkeypatch):
    ti = pkg()
    obs = ti.observables
    cfg = types.SimpleNamespace(observables={"descriptors": [["coord", 0]], "every": 2, "bins": 4, "bootstrap": 5})
    assert ti.drivers._observe_kw(cfg)["observe"] == {"descriptors": [["coord", 0]], "every": 2}
    seen = {}

    def fake_summary(cv, dl, bins=32, engine=None):
        return np.zeros((cv.shape[1], bins)), np.zeros((cv.shape[1], bins + 1)), 3.5

    def fake_bootstrap(logw, estimator, n_boot=1000, **kw):
        seen.update(logw=np.asarray(logw), estimator=estimator, n_boot=n_boot, kw=kw)
        return obs.BootstrapResult(3.5, (2.0, 4.0), np.arange(n_boot, dtype=np.float64), logw.shape[0])

    monkeypatch.setattr(obs, "end_state_summary", fake_summary)
    monkeypatch.setattr(obs, "bootstrap", fake_bootstrap)
    cvs = [np.zeros((3, 4, 1), np.float32), np.zeros((3, 2, 1), np.float32)]
    dlogps = [np.array([0.5, 1.0, -1.0, 2.0], np.float32), np.array([0.25, 0.0], np.float32)]
    ti.drivers._write_observables(cfg, str(tmp_path / "with.npz"), cvs, dlogps)
    z = np.load(tmp_path / "with.npz")
    assert sorted(z.files) == ["cv", "edges", "ess", "ess_boot", "ess_ci", "hist"]
    np.testing.assert_array_equal(z["ess_ci"], [2.0, 4.0])
    np.testing.assert_array_equal(z["ess_boot"], np.arange(5.0))
    np.testing.assert_array_equal(seen["logw"], -np.concatenate(dlogps))
    assert seen["logw"].dtype == np.float32 and seen["estimator"] == "ess" and seen["n_boot"] == 5 and seen["kw"] == {}
    # without the key: today's arrays in today's order, and no bootstrap call
    del cfg.observables["bootstrap"]
    seen["n_boot"] = 5
    ti.drivers._write_observables(cfg, str(tmp_path / "without.npz"), cvs, dlogps)
    z0 = np.load(tmp_path / "without.npz")
    assert sorted(z0.files) == ["cv", "edges", "ess", "hist"]
    assert z0.files == ["cv", "hist", "edges", "ess"] and z0["ess"].dtype == np.float64 and z0["ess"].shape == () and float(z0["ess"]) == 3.5
    assert seen["n_boot"] == 5                                     # the stand-in was not called again
    for bad in (0, -3, 2.5, True):
        cfg.observables["bootstrap"] = bad
        with pytest.raises(ValueError, match="bootstrap"):
            ti.drivers._write_observables(cfg, str(tmp_path / "bad.npz"), cvs, dlogps)
