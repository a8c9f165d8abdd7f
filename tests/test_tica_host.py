"""TICA without a GPU: the numpy restatement (tests/tica_numpy.py) against its second LAPACK route, the rank-deficient case, the pair
enumeration against a double loop, the Python argument checks, the header against ABI_SYMBOLS, the driver key's validation."""
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT, pkg
import tica_numpy as tn

LENGTHS = [3000, 2500, 1777, 920]
LAGS = [1, 4, 16]


def deficient_set():
    """x [n, 5] for encode = 0: three independent columns, a copy of the first, a constant -- rank 3 of 5"""
    x, off, _ = tn.synthetic(3, [700, 400, 333], seed=5)
    return np.concatenate([x, x[:, :1], np.full((len(x), 1), 0.75, np.float32)], axis=1), off


@pytest.mark.parametrize("K", [2, 8, 22, 32])
def test_restatement_against_the_generalized_route(K):
    """Full rank, both routes in fp64 LAPACK: eigenvalues to 1e-13, components to 1e-12 ||R_k|| / gap_k.  The smallest C00 eigenvalue is
    far above epsilon, so the whitening drops nothing."""
    x, off, _ = tn.synthetic(K, LENGTHS, seed=K)
    count, sm, cov = tn.moments(x, off, LAGS)
    d, dim = 2 * K, min(4, 2 * K)
    for l in range(len(LAGS)):
        _, C00, _ = tn.covariances(count[l], sm[l], cov[l])
        assert np.linalg.eigvalsh(C00)[0] > 0.05
        mu, ev, R, r = tn.fit(count[l], sm[l], cov[l], dim)
        mu2, ev2, R2, _ = tn.fit_generalized(count[l], sm[l], cov[l], dim)
        lam = tn.fit(count[l], sm[l], cov[l], d)[1]
        assert r == d and np.array_equal(mu, mu2) and np.all(np.diff(lam) <= 0) and lam[0] < 1
        assert np.abs(ev - ev2).max() <= 1e-13
        for k in range(dim):
            gap = np.abs(np.delete(lam, k) - lam[k]).min()
            assert gap > 1e-3
            assert np.abs(R[:, k] - R2[:, k]).max() <= 1e-12 * np.linalg.norm(R[:, k]) / gap
            f = int(np.argmax(np.abs(R[:, k])))
            assert R[f, k] > 0
        # the unscaled components are C00-orthonormal and diagonalise C0t
        _, C00, C0t = tn.covariances(count[l], sm[l], cov[l])
        W = tn.fit(count[l], sm[l], cov[l], dim, scaling=False)[2]
        np.testing.assert_allclose(W.T @ C00 @ W, np.eye(dim), atol=1e-10)
        np.testing.assert_allclose(W.T @ C0t @ W, np.diag(ev), atol=1e-10)
        np.testing.assert_array_equal(R, W * ev)


def test_rank_deficient_case():
    x, off = deficient_set()
    count, sm, cov = tn.moments(x, off, [2], enc=False)
    _, C00, _ = tn.covariances(count[0], sm[0], cov[0])
    s = np.linalg.eigvalsh(C00)
    assert not np.any((s > 1e-9) & (s < 1e-3))                     # nothing within a factor 1e3 of epsilon = 1e-6
    mu, ev, R, r = tn.fit(count[0], sm[0], cov[0], 5)
    assert r == 3 and np.all(np.isfinite(ev[:3])) and np.all(np.isnan(ev[3:]))
    assert np.all(np.isfinite(R[:, :3])) and np.all(np.isnan(R[:, 3:]))
    y = tn.transform(x, mu, R, enc=False)
    assert np.all(np.isfinite(y[:, :3])) and np.all(np.isnan(y[:, 3:]))


def test_pairs_against_a_double_loop():
    off = np.array([0, 5, 6, 9, 17, 20])
    for tau in (1, 2, 3, 4, 5, 8, 9):
        want = [i for t in range(len(off) - 1) for i in range(off[t], off[t + 1]) if i + tau < off[t + 1]]
        assert tn.pairs(off, tau).tolist() == want
    x, o, _ = tn.synthetic(2, [9, 4, 7], seed=1)
    count, sm, cov = tn.moments(x, o, [3])
    f = tn.encode(x)
    S = np.zeros((4, 4))
    for i in tn.pairs(o, 3):
        S += np.outer(f[i], f[i + 3])
    assert count[0] == 6 + 1 + 4
    np.testing.assert_allclose(cov[0, 2], S, atol=1e-14)


def test_end_to_end_recovers_the_slow_column_on_the_cpu():
    """the inputs of the GPU end-to-end test: |corr(tIC 1, well index of the slowest torsion)| >= 0.9 on the restatement"""
    x, off, wells = tn.synthetic(2, LENGTHS, seed=0)
    count, sm, cov = tn.moments(x, off, [64, 128])
    for l in range(2):
        mu, ev, R, _ = tn.fit(count[l], sm[l], cov[l], 2)
        y = tn.transform(x, mu, R)
        assert abs(np.corrcoef(y[:, 0], wells[:, 0])[0, 1]) >= 0.9


def test_python_argument_checks():
    obs = pkg().observables
    x = np.zeros((20, 3), np.float32)
    off = np.array([0, 12, 20])
    bad = [dict(values=np.zeros(20, np.float32)), dict(values=np.zeros((20, 33), np.float32)), dict(encode="cos"),
           dict(traj_offsets=[0, 12, 19]), dict(traj_offsets=[1, 12, 20]), dict(traj_offsets=[0, 12, 12, 20]), dict(traj_offsets=[0.0, 20.0]),
           dict(lags=[]), dict(lags=[0]), dict(lags=[1.5]), dict(lags=list(range(1, 34))), dict(lags=[11]), dict(lags=[[1]])]
    for kw in bad:
        args = dict(values=x, traj_offsets=off, lags=[1, 2], encode="torsion")
        args.update(kw)
        with pytest.raises(ValueError):
            obs.tica_moments(**args)
        with pytest.raises(ValueError):
            obs.tica_fit(**args)
    obs._check_tica_args(x, off, [10], "torsion")                   # 2 + 0 pairs: the least that is taken
    for kw in (dict(dim=0), dict(dim=7), dict(dim=True), dict(epsilon=-1.0), dict(epsilon=np.nan), dict(scaling="commute_map")):
        with pytest.raises(ValueError):
            obs.tica_fit(x, off, [1], **kw)
    with pytest.raises(ValueError):
        obs.tica_fit(np.zeros((20, 3), np.float32), off, [1], dim=4, encode="none")
    model = obs.TicaModel(np.array([1], np.int32), np.zeros((1, 6)), np.zeros((1, 2)), np.zeros((1, 6, 2)), np.array([6], np.int32),
                          np.zeros((1, 2)), "torsion")
    with pytest.raises(ValueError):
        obs.tica_transform(model, np.zeros((4, 2), np.float32))
    with pytest.raises(ValueError):
        obs.tica_transform(model, np.zeros(4, np.float32))
    for kw in (dict(bins=0), dict(bins=300), dict(range=(1.0, 1.0))):
        with pytest.raises(ValueError):
            obs.tica_marginals(model, x, **kw)
    ts = obs.tica_timescales([2, 4], np.array([[np.exp(-0.5), 1.0, -0.1], [0.5, np.nan, 0.0]]))
    np.testing.assert_allclose(ts[0, 0], 4.0)
    np.testing.assert_allclose(ts[1, 0], -4.0 / np.log(0.5))
    assert np.isnan(ts[0, 1:]).all() and np.isnan(ts[1, 1:]).all()


def test_header_and_abi_symbols_name_the_entry_points():
    ti = pkg()
    text = open(os.path.join(ROOT, "include", "ti_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(ti_obs_tica_[a-z_0-9]+)\s*\(", text))
    assert declared == {"ti_obs_tica_moments", "ti_obs_tica_fit", "ti_obs_tica_transform"}
    assert declared <= set(ti._lib.ABI_SYMBOLS)
    assert int(re.search(r"#define TI_TICA_MAX_LAGS (\d+)", text).group(1)) == ti._lib.TICA_MAX_LAGS == 32
    assert int(re.search(r"#define TI_TICA_MAX_K (\d+)", text).group(1)) == ti._lib.TICA_MAX_K == 32
    assert int(re.search(r"#define TI_ABI_VERSION (\d+)", text).group(1)) == 5
    import ctypes
    assert ctypes.sizeof(ti._lib.TicaDesc) == 24


def test_c_abi_refusals_that_need_no_device():
    """every TI_E_ARG that comes before the handle is looked at, through a NULL handle"""
    import ctypes as C
    ti = pkg()
    ti.build.build()
    L, lib = ti._lib.lib(), ti._lib
    x = np.zeros((20, 3), np.float32)
    off, lags = np.array([0, 12, 20], np.int64), np.array([1, 2], np.int32)
    count, sm, cov = np.zeros(2, np.int64), np.zeros((2, 2, 6)), np.zeros((2, 3, 6, 6))
    p = lambda a: C.c_void_p(a.ctypes.data)
    i64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))

    def mom(values=x, stride=3, cstride=1, n=20, K=3, enc=1, off=off, n_traj=2, lags=lags, n_lag=2, count=count, mem=0):
        return L.ti_obs_tica_moments(None, None if values is None else p(values), stride, cstride, n, K, enc, None if off is None else i64(off),
                                     n_traj, None if lags is None else lib.iptr(lags), n_lag, None if count is None else p(count), p(sm), p(cov), mem)

    assert mom() == lib.TI_E_ARG and "NULL handle" in lib.last_error()
    for kw, word in ((dict(values=None), "values"), (dict(mem=7), "mem"), (dict(K=0), "K"), (dict(K=33), "K"), (dict(enc=2), "encode"),
                     (dict(cstride=0), "cstride"), (dict(stride=2), "stride"), (dict(n=0), "row count"), (dict(off=None), "NULL"),
                     (dict(lags=None), "NULL"), (dict(count=None), "NULL"), (dict(n_lag=0), "n_lag"), (dict(n_lag=33), "n_lag"),
                     (dict(n_traj=0), "n_traj"), (dict(off=np.array([0, 12, 19], np.int64)), "traj_off"),
                     (dict(off=np.array([0, 0, 20], np.int64)), "ascending"), (dict(lags=np.array([1, 0], np.int32)), "lag 1"),
                     (dict(lags=np.array([1, 11], np.int32)), "lag 11")):
        assert mom(**kw) == lib.TI_E_ARG and word in lib.last_error(), (kw, lib.last_error())
    # K = 32 without encoding is fine, with it d = 64 is the limit; nothing above it exists for K <= 32
    desc = lib.TicaDesc(2, 1, 0, 1e-6)
    mean, ev, comp, rank = np.zeros((2, 6)), np.zeros((2, 2)), np.zeros((2, 6, 2)), np.zeros(2, np.int32)

    def fit(d=6, n_lag=2, desc=desc, mem=0, count=count):
        return L.ti_obs_tica_fit(None, None if count is None else p(count), p(sm), p(cov), n_lag, d, None if desc is None else C.byref(desc), p(mean),
                                 p(ev), p(comp), p(rank), mem)

    assert fit() == lib.TI_E_ARG and "NULL handle" in lib.last_error()
    for kw, word in ((dict(count=None), "NULL"), (dict(desc=None), "NULL"), (dict(mem=3), "mem"), (dict(n_lag=0), "n_lag"), (dict(d=0), "d must"),
                     (dict(d=65), "d must"), (dict(desc=lib.TicaDesc(0, 1, 0, 1e-6)), "dim"), (dict(desc=lib.TicaDesc(7, 1, 0, 1e-6)), "dim"),
                     (dict(desc=lib.TicaDesc(2, 2, 0, 1e-6)), "scaling"), (dict(desc=lib.TicaDesc(2, 1, 1, 1e-6)), "reserved"),
                     (dict(desc=lib.TicaDesc(2, 1, 0, -1.0)), "epsilon"), (dict(desc=lib.TicaDesc(2, 1, 0, float("nan"))), "epsilon")):
        assert fit(**kw) == lib.TI_E_ARG and word in lib.last_error(), (kw, lib.last_error())
    out = np.zeros((2, 20, 2), np.float32)

    def tr(K=3, enc=1, d=6, dim=2, n_lag=2, B=20, stride=3, mem=0):
        return L.ti_obs_tica_transform(None, p(x), stride, 1, B, K, enc, p(mean), p(comp), n_lag, d, dim, p(out), mem)

    assert tr() == lib.TI_E_ARG and "NULL handle" in lib.last_error()
    for kw, word in ((dict(d=3), "d must"), (dict(enc=0), "d must"), (dict(dim=0), "dim"), (dict(dim=7), "dim"), (dict(n_lag=33), "n_lag"),
                     (dict(B=0), "row count"), (dict(stride=1), "stride"), (dict(mem=2), "mem")):
        assert tr(**kw) == lib.TI_E_ARG and word in lib.last_error(), (kw, lib.last_error())


def tica_config(tmp_path, **over):
    A = 6
    traj = np.full((8, 40, A, 3), np.nan, np.float32)
    traj[0] = np.random.RandomState(0).standard_normal((40, A, 3))
    path = str(tmp_path / "traj.npy")
    np.save(path, traj)
    key = dict(traj=path, n_frames=10, temperature=300, lags=[1, 2])
    key.update(over.pop("key", {}))
    o = {"descriptors": [["dist", 0, 1]], "zmatrix": {"bonds": [[0, 1], [1, 2], [2, 3], [3, 4], [4, 5]]}, "tica": key}
    o.update(over)
    return types.SimpleNamespace(observables={k: v for k, v in o.items() if v is not None})


def test_driver_key_validation(tmp_path):
    drv = pkg().drivers
    t = drv._check_tica(tica_config(tmp_path))
    assert t["frames"].shape == (40, 6, 3) and t["traj_off"].tolist() == [0, 10, 20, 30, 40] and t["lags"].tolist() == [1, 2]
    assert (t["dim"], t["bins"], t["range"], t["epsilon"]) == (2, 80, (-2.5, 2.5), 1e-6)
    assert drv._check_tica(types.SimpleNamespace(observables={"descriptors": [["dist", 0, 1]]})) is None
    assert drv._check_tica(types.SimpleNamespace()) is None
    for driver in ("sample_latent", "sample_adw"):
        with pytest.raises(ValueError, match="sample_ambient"):
            drv._check_tica(tica_config(tmp_path), driver)
    for over in (dict(zmatrix=None), dict(descriptors=None), dict(key=dict(temperature=400)), dict(key=dict(temperature=350)),
                 dict(key=dict(n_frames=7)), dict(key=dict(n_frames=0)), dict(key=dict(lags=[])), dict(key=dict(lags=[10])), dict(key=dict(lags=[0])),
                 dict(key=dict(lags=[1.5])), dict(key=dict(dim=0)), dict(key=dict(dim=7)), dict(key=dict(bins=0)), dict(key=dict(range=[1, 1])),
                 dict(key=dict(epsilon=-1)), dict(key=dict(traj=str(tmp_path / "none.npy"))), dict(key=dict(window=3)),
                 dict(key=dict(lags=list(range(1, 10)) * 4))):
        with pytest.raises(ValueError, match="tica"):
            drv._check_tica(tica_config(tmp_path, **over))
    for missing in ("traj", "n_frames", "temperature", "lags"):
        cfg = tica_config(tmp_path)
        del cfg.observables["tica"][missing]
        with pytest.raises(ValueError, match="tica"):
            drv._check_tica(cfg)
    # the key is popped where the other observable keys are: the observer's arguments do not see it
    kw = drv._observe_kw(tica_config(tmp_path))
    assert set(kw["observe"]) == {"descriptors"}
