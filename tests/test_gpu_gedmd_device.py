"""ti_obs_gedmd_spectrum on the GPU (observables.gedmd_spectrum / gedmd_generator with solver="device"): the reference's eigenvalues
and ranks through the recorded index rows (tests/golden/gedmd_reference.npz) under the host route's own tolerances, the edge orders
of the second solve, the device route against the host route on the generator path, and where the results live.

Edge orders are compared with the host route on the same Gram matrix.  Their bound: both routes solve the whitened problem
R = L^H ML L with ||L||^2 = 1 / lambda_r (the smallest kept eigenvalue of G); an eigensolver's backward error p eps ||G|| on G moves
L relatively by p eps cond, cond = lambda_0 / lambda_r, and R's eigenvalues by that times ||R|| <= ||ML|| / lambda_r.  With the factor
64 the project allows between two LAPACK builds: 64 p 2^-53 cond ||ML||_2 / lambda_r."""
import numpy as np
import pytest

from conftest import pkg
import gedmd_numpy as gn
from test_gedmd_host import fixture_cases

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def eng():
    return pkg().observables._service_engine(0)


def ml_of(G, omega, a):
    return -0.5 * a * (omega.T @ omega) * G


def check_vectors(G, omega, a, d, W):
    """the host test's own tolerances: W^H G W = 1 to 1e-7, W^H ML W = diag(d) to 1e-6"""
    np.testing.assert_allclose(W.conj().T @ G @ W, np.eye(len(d)), atol=1e-7)
    np.testing.assert_allclose(W.conj().T @ ml_of(G, omega, a) @ W, np.diag(d), atol=1e-6)


def test_fixture_rows_reproduce_the_reference(eng):
    obs = pkg().observables
    cases, ev_dev = fixture_cases()
    worst = 0.0
    for c in cases:
        res = obs.gedmd_generator(c["x"], c["omega"], c["nev"], c["a"], tol=c["tol"], n_boot=3, indices=c["idx"], engine=eng, solver="device")
        got = np.concatenate([res.eigenvalues[None], res.estimates])
        worst = max(worst, np.abs(got - c["ev"]).max())
        print(f"{c['name']}: worst eigenvalue difference {np.abs(got - c['ev']).max():.2e}")
        assert np.abs(got - c["ev"]).max() <= 64 * ev_dev, (c["name"], np.abs(got - c["ev"]).max())
        assert res.rank == c["rank"][0] and res.eigenvectors.shape == (c["p"], c["nev"]) and res.ci.shape == (2, c["nev"])
        G = obs.rff_gram(c["x"], c["omega"], n_boot=3, indices=c["idx"], engine=eng)
        d, W, r = obs.gedmd_spectrum(G, c["omega"], c["a"], c["nev"], c["tol"], solver="device", engine=eng)
        assert d.shape == (4, c["nev"]) and W.shape == (4, c["p"], c["nev"]) and r.shape == (4,) and W.dtype == np.complex128
        np.testing.assert_array_equal(r, c["rank"])
        assert np.array_equal(d[0], res.eigenvalues) and np.array_equal(d[1:], res.estimates)
        for i in range(4):
            check_vectors(G[i], c["omega"], c["a"], d[i], W[i])
    print(f"device route against the reference: worst eigenvalue difference {worst:.2e} = {worst / ev_dev:.2f} ev_dev (allowed 64)")


def edge_bound(G, omega, a, r):
    lam = np.linalg.eigvalsh(G)[::-1]
    return 64 * G.shape[0] * EPS * (lam[0] / lam[r - 1]) * np.linalg.norm(ml_of(G, omega, a), 2) / lam[r - 1]


# (name, n, d, p, nev, tol, sigma)
EDGES = [("nev1", 65, 1, 8, 1, 1e-4, 0.1), ("nev-p", 65, 1, 8, 8, 1e-4, 0.1), ("rmin", 65, 1, 8, 4, 0.5, 0.6), ("p1", 33, 1, 1, 1, 1e-4, 0.6),
         ("p63-full", 2000, 16, 63, 4, 0.0, 2.0), ("p64-full", 2000, 16, 64, 4, 0.0, 2.0)]


@pytest.mark.parametrize("name,n,d,p,nev,tol,sigma", EDGES)
def test_edge_orders_against_the_host_route(eng, name, n, d, p, nev, tol, sigma):
    obs = pkg().observables
    rs = np.random.RandomState(n + p)
    x = rs.standard_normal((n, d)).astype(np.float32)
    omega = obs.sample_rff_gaussian(d, p, sigma, 3)
    G = obs.rff_gram(x, omega, engine=eng)[0]
    dh, Wh, rh = obs.gedmd_spectrum(G, omega, 1.6, nev, tol)
    dd, Wd, rd = obs.gedmd_spectrum(G, omega, 1.6, nev, tol, solver="device", engine=eng)
    assert dd.shape == (nev,) and Wd.shape == (p, nev) and rd.shape == () and int(rd) == int(rh)
    if name.endswith("full"):
        assert int(rd) == p
    if name == "rmin":                                             # fewer than nev pass the harsh cutoff: nev are kept
        sv = np.sqrt(np.maximum(np.linalg.eigvalsh(G)[::-1], 0.0))
        assert (sv / sv[0] >= tol).sum() < nev and int(rd) == nev
    b = edge_bound(G, omega, 1.6, int(rh))
    print(f"{name}: rank {int(rd)}, |device - host| {np.abs(dd - dh).max():.2e}, bound {b:.2e}")
    assert np.abs(dd - dh).max() <= b
    check_vectors(G, omega, 1.6, dd, Wd)


def test_device_route_against_host_route_on_the_generator_path(eng):
    """n = 4096, p = 50, d = 1, tol = 1e-4, nev = 4, 400 resamples, seed 7.  A row where the host route has a singular ratio within
    1e-6 relative of tol is left out (the two routes may then decide the rank differently): at most 1 % of the rows."""
    obs = pkg().observables
    _, ev_dev = fixture_cases()
    rs = np.random.RandomState(2024)
    x = (np.where(rs.random_sample(4096) < 0.5, -1.0, 1.0) + 0.35 * rs.standard_normal(4096)).astype(np.float32)
    omega = obs.sample_rff_gaussian(1, 50, 0.6, 1)
    tol = 1e-4
    host = obs.gedmd_generator(x, omega, 4, 1.6, tol=tol, n_boot=400, seed=7, engine=eng)
    dev = obs.gedmd_generator(x, omega, 4, 1.6, tol=tol, n_boot=400, seed=7, engine=eng, solver="device")
    G = obs.rff_gram(x, omega, n_boot=400, seed=7, engine=eng)
    s = np.sqrt(np.maximum(np.linalg.eigvalsh(G)[:, ::-1], 0.0))
    keep = (np.abs(s / s[:, :1] / tol - 1.0) > 1e-6).all(axis=1)
    assert keep.shape == (401,) and (~keep).sum() <= 4, (~keep).sum()
    _, _, rh = obs.gedmd_spectrum(G, omega, 1.6, 4, tol)
    _, _, rd = obs.gedmd_spectrum(G, omega, 1.6, 4, tol, solver="device", engine=eng)
    np.testing.assert_array_equal(rd[keep], rh[keep])
    eh, ed = np.concatenate([host.eigenvalues[None], host.estimates])[keep], np.concatenate([dev.eigenvalues[None], dev.estimates])[keep]
    diff = np.abs(ed - eh).max()
    ci = [np.percentile(e[1:] if keep[0] else e, [2.5, 97.5], axis=0) for e in (eh, ed)]
    print(f"rows left out {(~keep).sum()}, worst eigenvalue difference {diff:.2e} = {diff / ev_dev:.2f} ev_dev, intervals differ by {np.abs(ci[0] - ci[1]).max():.2e}")
    assert diff <= 64 * ev_dev
    assert np.abs(ci[0] - ci[1]).max() <= 64 * ev_dev
    if keep.all():
        assert np.abs(host.ci - dev.ci).max() <= 64 * ev_dev and dev.rank == host.rank


def test_a_cuda_gram_stack_and_its_numpy_copy_give_the_same_bits(eng):
    import torch
    obs = pkg().observables
    c = fixture_cases()[0][1]
    Gd = obs.rff_gram(torch.from_numpy(c["x"]).cuda(), c["omega"], n_boot=3, indices=torch.from_numpy(c["idx"]).cuda(), engine=eng)
    assert Gd.is_cuda
    out_d = obs.gedmd_spectrum(Gd, c["omega"], c["a"], c["nev"], c["tol"], solver="device", engine=eng)
    out_h = obs.gedmd_spectrum(Gd.cpu().numpy(), c["omega"], c["a"], c["nev"], c["tol"], solver="device", engine=eng)
    for a, b in zip(out_d, out_h):
        assert isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    ev, vec, rank = eng.gedmd_spectrum(Gd, c["omega"], c["a"], c["nev"], c["tol"])            # the engine call keeps them on the GPU
    assert ev.is_cuda and vec.is_cuda and rank.is_cuda and np.array_equal(ev.cpu().numpy(), out_d[0])


def test_degenerate_input_gives_nan_and_p_65_raises(eng):
    ti = pkg()
    obs = ti.observables
    omega = obs.sample_rff_gaussian(1, 4, 0.6, 0)
    G = np.stack([np.eye(4, dtype=np.complex128), np.zeros((4, 4), np.complex128), np.diag([3.0, 2.0, 0.0, 0.0]).astype(np.complex128)])
    d, W, r = obs.gedmd_spectrum(G, omega, 1.6, 2, tol=0.0, solver="device", engine=eng)
    assert np.isfinite(d[0]).all() and np.isfinite(W[0]).all() and r[0] == 4
    assert np.isnan(d[1:]).all() and np.isnan(W[1:]).all()                                  # not an error
    with pytest.raises(ValueError, match="64"):
        obs.gedmd_spectrum(np.eye(65, dtype=np.complex128), np.ones((1, 65)), 1.6, 2, solver="device", engine=eng)
    bad = G.copy()
    bad[2, 0, 3] = np.nan
    with pytest.raises(ti._lib.TiError, match="Gram matrix 2") as ei:
        obs.gedmd_spectrum(bad, omega, 1.6, 2, solver="device", engine=eng)
    assert ei.value.code == ti._lib.TI_E_NAN
