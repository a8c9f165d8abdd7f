"""sample_ambient with and without the `tica` key of config.observables, on the synthetic species the other driver tests use: the
arrays the key adds, their shapes, the model against the numpy restatement on the same torsions, and every other file and array of a
run without the key left as it is."""
import os
import types

import numpy as np
import pytest

from conftest import pkg
import tica_numpy as tn
import zmat_numpy as zn

pytestmark = pytest.mark.gpu


def test_sample_ambient_with_the_tica_key(tmp_path):
    ti = pkg()
    A, n, bins, n_rep, n_frames = 9, 7, 16, 4, 30
    rs = np.random.RandomState(1)
    traj = rs.standard_normal((8, n, A, 3)) * 0.3
    os.makedirs(tmp_path / "test")
    np.save(tmp_path / "test" / "00031.npy", traj)
    md = np.full((8, n_rep * n_frames, A, 3), np.nan, np.float32)                  # only 300 K was simulated
    md[0] = (rs.standard_normal((1, A, 3)) + 0.2 * np.cumsum(rs.standard_normal((n_rep * n_frames, A, 3)), axis=0)).astype(np.float32)
    np.save(tmp_path / "md.npy", md)
    ds = ti.data.MDQM9SamplerDataset("00031.npy", str(tmp_path), "test", T0=1000, T1=300, scale=False, cutoff=1000)
    b = ti.thermo.ambient.cPaiNN(n_features=32, score_layers=1, temp_length=100)
    b.load_state_dict(ti.synthetic.painn_state_dict(0, 32, 1, 25, 4))
    bonds = [[i, i + 1] for i in range(A - 1)] + [[2, 7]]
    obs = {"descriptors": [["dist", 0, 1]], "bins": 4, "zmatrix": {"bonds": bonds, "root": 3, "bins": 8, "length_range": [0.0, 12.0]}}
    common = dict(seed=0, batch_size=3, n_steps=3, atol=1e-5, rtol=1e-5, return_dlogp=1, method="euler")
    plain = types.SimpleNamespace(**common, data_save_path=str(tmp_path / "plain"), data_save_name="r", observables=obs)
    ti.drivers.sample_ambient(plain, b, ds)
    key = {"traj": str(tmp_path / "md.npy"), "n_frames": n_frames, "temperature": 300, "lags": [1, 3], "bins": bins, "range": [-3.0, 3.0]}
    cfg = types.SimpleNamespace(**common, data_save_path=str(tmp_path / "keyed"), data_save_name="r", observables={**obs, "tica": key})
    ti.drivers.sample_ambient(cfg, b, ds)
    with pytest.raises(ValueError, match="not finite"):                           # a temperature that was not simulated, before the rollout
        ti.drivers.sample_ambient(types.SimpleNamespace(**common, data_save_path=str(tmp_path / "bad"), data_save_name="r",
                                                        observables={**obs, "tica": {**key, "temperature": 400}}), b, ds)
    np.save(tmp_path / "md10.npy", np.concatenate([md, md[:, :, :1]], axis=2))    # one atom more than the zmatrix key's topology
    with pytest.raises(ValueError, match="atoms"):                                # also before the rollout
        ti.drivers.sample_ambient(types.SimpleNamespace(**common, data_save_path=str(tmp_path / "bad"), data_save_name="r",
                                                        observables={**obs, "tica": {**key, "traj": str(tmp_path / "md10.npy")}}), b, ds)
    assert not os.path.exists(tmp_path / "bad")
    files = sorted(os.listdir(tmp_path / "plain"))
    assert sorted(os.listdir(tmp_path / "keyed")) == files
    for f in files:
        if f.endswith(".npy"):                     # the key changes no other file
            assert open(tmp_path / "plain" / f, "rb").read() == open(tmp_path / "keyed" / f, "rb").read(), f
    added = ["tica_lags", "tica_eigenvalues", "tica_timescales", "tica_rank", "tica_mean", "tica_components", "tica_hist_md", "tica_hist_0",
             "tica_hist_1", "tica_edges"]
    K = A - 3
    with np.load(tmp_path / "plain" / "observables_r.npz") as z0, np.load(tmp_path / "keyed" / "observables_r.npz") as z:
        assert z.files == z0.files + added
        for k in z0.files:
            np.testing.assert_array_equal(z[k], z0[k])
        assert z["tica_lags"].tolist() == [1, 3] and z["tica_rank"].tolist() == [2 * K, 2 * K]
        assert z["tica_mean"].shape == (2, 2 * K) and z["tica_components"].shape == (2, 2 * K, 2) and z["tica_eigenvalues"].shape == (2, 2)
        np.testing.assert_array_equal(z["tica_edges"], np.linspace(-3.0, 3.0, bins + 1))
        order, ref = zn.from_bonds(bonds, A, 3)
        tor = zn.construct(md[0], order, ref)[:, 2:, 2].astype(np.float32)
        off = np.arange(0, n_rep * n_frames + 1, n_frames)
        count, sm, cov = tn.moments(tor, off, [1, 3])
        for l in range(2):
            mu, ev, R, r = tn.fit(count[l], sm[l], cov[l], 2)
            # the device's torsions differ from the restatement's in the last fp32 digits; the eigenvalues move by as much
            np.testing.assert_allclose(z["tica_eigenvalues"][l], ev, rtol=0, atol=1e-4)
            np.testing.assert_allclose(z["tica_mean"][l], mu, rtol=0, atol=1e-5)
        lam = z["tica_eigenvalues"]
        want = np.where((lam > 0) & (lam < 1), -np.array([[1.0], [3.0]]) / np.log(np.where((lam > 0) & (lam < 1), lam, 0.5)), np.nan)
        np.testing.assert_array_equal(z["tica_timescales"], want)
        for name in ("tica_hist_md", "tica_hist_0", "tica_hist_1"):
            h = z[name]
            assert h.shape == (2, 2, bins) and h.dtype == np.float64 and np.all(h >= 0) and np.all(h.sum(axis=2) <= 1 + 1e-12)
        # the fitted frames projected on their own unit-variance components: nearly all of the mass lies inside +-3
        assert np.all(z["tica_hist_md"].sum(axis=2) > 0.9)
