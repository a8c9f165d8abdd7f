"""sample_ambient with and without the `zmatrix` key of config.observables, on the synthetic species the other driver tests use: the
arrays the key adds, their shapes, the reference's slices, the weighted end-state marginals with the IQR mask, and the files of a run
without the key left as they are."""
import os
import types

import numpy as np
import pytest

from conftest import pkg
import obs_numpy as on
import zmat_numpy as zn

pytestmark = pytest.mark.gpu


def test_sample_ambient_with_the_zmatrix_key(tmp_path):
    ti = pkg()
    A, n, scale, bins = 9, 7, 0.25, 8
    traj = np.random.RandomState(1).standard_normal((8, n, A, 3)) * 0.3
    os.makedirs(tmp_path / "test")
    np.save(tmp_path / "test" / "00031.npy", traj)
    ds = ti.data.MDQM9SamplerDataset("00031.npy", str(tmp_path), "test", T0=1000, T1=300, scale=False, cutoff=1000)
    b = ti.thermo.ambient.cPaiNN(n_features=32, score_layers=1, temp_length=100)
    b.load_state_dict(ti.synthetic.painn_state_dict(0, 32, 1, 25, 4))
    obs = {"descriptors": [["dist", 0, 1], ["torsion", 0, 1, 2, 3]], "bins": 4}
    common = dict(seed=0, batch_size=3, n_steps=3, atol=1e-5, rtol=1e-5, return_dlogp=1, method="euler")
    plain = types.SimpleNamespace(**common, data_save_path=str(tmp_path / "plain"), data_save_name="r", observables=obs)
    ti.drivers.sample_ambient(plain, b, ds)
    bonds = [[i, i + 1] for i in range(A - 1)] + [[2, 7]]
    cfg = types.SimpleNamespace(**common, data_save_path=str(tmp_path / "keyed"), data_save_name="r",
                                observables={**obs, "zmatrix": {"bonds": bonds, "root": 3, "bins": bins, "length_range": [0.0, 12.0], "scale": scale}})
    samples, _ = ti.drivers.sample_ambient(cfg, b, ds)
    files = ["dlogps_r.npy", "latent_dlogps_r.npy", "latent_noises_r.npy", "observables_r.npz", "samples_r.npy"]
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(os.listdir(tmp_path / "keyed")) == files
    for f in files:
        if f.endswith(".npy"):                     # the key changes no other file
            assert open(tmp_path / "plain" / f, "rb").read() == open(tmp_path / "keyed" / f, "rb").read(), f
    added = ["torsions_0", "torsions_1", "bond_angles_0", "bond_angles_1", "bond_lengths_0", "bond_lengths_1", "zmat_marginals_0",
             "zmat_marginals_1", "zmat_ranges"]
    with np.load(tmp_path / "plain" / "observables_r.npz") as z0, np.load(tmp_path / "keyed" / "observables_r.npz") as z:
        assert z0.files == ["cv", "hist", "edges", "ess"] and z.files == z0.files + added
        for k in z0.files:
            np.testing.assert_array_equal(z[k], z0[k])
        order, ref = zn.from_bonds(bonds, A, 3)
        for tag, frame in (("0", 0), ("1", -1)):
            want = zn.construct(samples[:, frame] / scale, order, ref)           # fp32 / python float stays fp32, as in results_00031.py
            for name, sl in (("torsions", want[:, 2:, 2]), ("bond_angles", want[:, 1:, 1]), ("bond_lengths", want[:, :, 0])):
                got = z[f"{name}_{tag}"]
                assert got.shape == sl.shape and got.dtype == np.float32
                assert (np.abs(got - sl) <= 1e-6 * (1 + np.abs(sl))).all(), (name, tag)
            assert z[f"torsions_{tag}"].shape == (n, A - 3) and z[f"bond_angles_{tag}"].shape == (n, A - 2)
            assert z[f"bond_lengths_{tag}"].shape == (n, A - 1)
            m = z[f"zmat_marginals_{tag}"]
            assert m.shape == (3 * A - 6, bins) and m.dtype == np.float64
            cols = np.concatenate([z[f"bond_lengths_{tag}"], z[f"bond_angles_{tag}"], z[f"torsions_{tag}"]], axis=1)
            for j in range(3 * A - 6):             # unweighted: no energy key
                h0, _ = on.weighted_histogram(cols[:, j], None, bins, *z["zmat_ranges"][j])
                assert np.abs(m[j] - h0).max() <= 1e-12 * n
        np.testing.assert_array_equal(z["zmat_ranges"][[0, A - 1, 2 * A - 3]], [[0.0, 12.0], [0.0, np.pi], [-np.pi, np.pi]])


def test_weighted_marginals_with_the_iqr_mask():
    """the arrays of a run whose energy key supplies logw: the x0 marginals unweighted, the end state's weighted and filtered"""
    ti = pkg()
    dr = ti.drivers
    rs = np.random.RandomState(3)
    A, B = 5, 400
    zm = ti.zmatrix.ZMatrix.from_bonds([[0, 1], [1, 2], [2, 3], [3, 4]], A)
    z = np.zeros((2, B, A - 1, 3), np.float32)
    z[..., 0] = rs.uniform(0.9, 1.6, (2, B, A - 1))
    z[:, :, 1:, 1] = rs.uniform(0.1, 3.0, (2, B, A - 2))
    z[:, :, 2:, 2] = rs.uniform(-3.1, 3.1, (2, B, A - 3))
    logw = (rs.standard_normal(B) * 2.0).astype(np.float32)
    logw[::40] += 7.0
    g = dict(zm=zm, bins=16, length_range=(0.5, 2.0), scale=1.0, iqr_k=1.5)
    out = dr._zmatrix_arrays(g, z[0], z[1], logw)
    keep = zn.iqr_keep(logw, 1.5)
    assert 0 < keep.sum() < B
    np.testing.assert_array_equal(out["zmat_keep"], keep)
    cols = ti.zmatrix.marginal_columns(A)
    sel = keep != 0
    for j, c in enumerate(cols):
        lo, hi = out["zmat_ranges"][j]
        h0, _ = on.weighted_histogram(z[0].reshape(B, -1)[:, c], None, 16, lo, hi)
        h1, _ = on.weighted_histogram(z[1].reshape(B, -1)[sel, c], logw[sel], 16, lo, hi)
        assert np.abs(out["zmat_marginals_0"][j] - h0).max() <= 1e-12 * B
        assert np.abs(out["zmat_marginals_1"][j] - h1).max() <= 1e-12 * B
    np.testing.assert_array_equal(out["torsions_1"], z[1][:, 2:, 2])
    no_mask = dr._zmatrix_arrays({**g, "iqr_k": None}, z[0], z[1], logw)
    assert "zmat_keep" not in no_mask
    h1, _ = on.weighted_histogram(z[1].reshape(B, -1)[:, 0], logw, 16, 0.5, 2.0)
    assert np.abs(no_mask["zmat_marginals_1"][0] - h1).max() <= 1e-12 * B
