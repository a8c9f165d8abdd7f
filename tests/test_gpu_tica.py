"""TICA on the GPU (ti_obs_tica_moments, ti_obs_tica_fit, ti_obs_tica_transform) against the fp64 numpy restatement of
tests/tica_numpy.py: the moments under the entrywise bound of ``moments_bound`` at the edges of the contraction kernel, their
determinism, the model algebra fed the restatement's moments, the projection, the public functions end to end, the refusals.

Feature counts: d = K without the encoding (K <= 32) and d = 2 K with it, so the d = 33 of an odd count above 32 does not exist; the
cases take d = 34 in its place, which is the same build of the kernel (three column tiles, the last one partly pad)."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg
import tica_numpy as tn
from test_tica_host import LAGS, LENGTHS, deficient_set

pytestmark = pytest.mark.gpu
S = 8192
worst = {"moments": 0.0}


@pytest.fixture(scope="module")
def eng():
    return pkg().observables._service_engine(0)


def check_moments(eng, x, off, lags, enc, name):
    """device against restatement under the entrywise bound; exact counts and symmetry; returns the device's arrays"""
    count, sm, cov = eng.tica_moments(x, off, np.asarray(lags, np.int32), enc)
    rc, rs, rv = tn.moments(x, off, lags, enc)
    bs, bv = tn.moments_bound(x, off, lags, enc)
    assert count.dtype == np.int64 and np.array_equal(count, rc), name
    assert np.array_equal(cov[:, 0], cov[:, 0].transpose(0, 2, 1)) and np.array_equal(cov[:, 1], cov[:, 1].transpose(0, 2, 1)), name
    assert np.isfinite(sm).all() and np.isfinite(cov).all(), name
    with np.errstate(invalid="ignore", divide="ignore"):          # an entry whose bound is 0 has to be exact
        frac = max(np.max(np.where(bs > 0, np.abs(sm - rs) / bs, np.where(sm == rs, 0.0, np.inf))),
                   np.max(np.where(bv > 0, np.abs(cov - rv) / bv, np.where(cov == rv, 0.0, np.inf))))
    worst["moments"] = max(worst["moments"], frac)
    print(f"{name}: worst |device - restatement| / bound {frac:.3f} (so far {worst['moments']:.3f})")
    assert frac <= 1.0, (name, frac)
    return count, sm, cov


# (K, encode): d = 1, 2, 15, 16, 17, 32 plain and d = 2, 16, 32, 34, 44, 64 encoded
WIDTHS = [(1, 0), (2, 0), (15, 0), (16, 0), (17, 0), (32, 0), (1, 1), (8, 1), (16, 1), (17, 1), (22, 1), (32, 1)]


@pytest.mark.parametrize("K,enc", WIDTHS)
def test_moments_feature_counts(eng, K, enc):
    """Every tile count of the kernel (1 .. 4 column tiles, with and without pad columns), three ragged trajectories, two lags.
    Worst observed fraction of the bound over this file's moment tests: see test_moments_pair_counts."""
    x, off, _ = tn.synthetic(K, [300, 41, 77], seed=100 + K)
    check_moments(eng, x, off, [1, 7], enc, f"K={K} enc={enc}")


def test_moments_pair_counts(eng):
    """One trajectory of 2 S + 2 frames; the lag 2 S + 2 - N leaves N pairs: N = 2, 3, 15, 16, 17, 63, 64, 65 (K steps and fills),
    S - 1, S, S + 1 (one segment, exactly one, one pair into the second), 2 S + 1 (three segments).  Twelve lags in one call.
    Worst observed fraction of the bound on an MI355X, over all moment tests of this file: 0.038 (K = 1 without the encoding)."""
    counts = [2, 3, 15, 16, 17, 63, 64, 65, S - 1, S, S + 1, 2 * S + 1]
    x, off, _ = tn.synthetic(3, [2 * S + 2], seed=7)
    count, _, _ = check_moments(eng, x, off, [2 * S + 2 - n for n in counts], 1, "pair counts")
    assert count.tolist() == counts


def test_moments_boundaries(eng):
    """Trajectory boundaries inside a 4-pair K step and inside a 16-pair fill; a segment boundary exactly at a trajectory boundary and
    inside a trajectory; trajectories of length tau - 1, tau (no pair) and tau + 1 (one pair)."""
    x, off, _ = tn.synthetic(5, [6, 9, 23, 40], seed=8)                      # pairs at lag 1: 5, 8, 22, 39
    check_moments(eng, x, off, [1, 2], 1, "boundaries in a K step / fill")
    x, off, _ = tn.synthetic(2, [S + 1, 100, S + 50], seed=9)                # lag 1: S pairs, then 99, then S + 49
    count, _, _ = check_moments(eng, x, off, [1, 50], 1, "segment boundaries")
    assert count[0] == 2 * S + 148
    x, off, _ = tn.synthetic(4, [4, 5, 6, 30, 5, 4], seed=10)
    count, _, _ = check_moments(eng, x, off, [5], 0, "short trajectories")
    assert count[0] == 1 + 25


def test_moments_32_lags(eng):
    x, off, _ = tn.synthetic(6, [100, 77], seed=11)
    count, _, _ = check_moments(eng, x, off, list(range(1, 33)), 1, "32 lags")
    assert count.tolist() == [177 - 2 * t for t in range(1, 33)]


def test_moments_determinism(eng):
    """The same bits from host and device memory, for a lag alone and inside a list, for a call repeated, and for strided values
    (the torsion column of a NaN-filled [n, K + 2, 3] array, whose other entries are never read) and a contiguous copy."""
    import torch
    x, off, _ = tn.synthetic(22, [S + 700, 901, 333], seed=12)
    lags = np.array([1, 3, 1000], np.int32)
    ref = eng.tica_moments(x, off, lags, 1)
    again = eng.tica_moments(x, off, lags, 1)
    xd = torch.as_tensor(x).cuda()
    dev = eng.tica_moments(xd, off, lags, 1)
    assert all(hasattr(a, "data_ptr") and a.is_cuda for a in dev)
    for a, b, c in zip(ref, again, dev):
        assert np.array_equal(a, b) and np.array_equal(a, c.cpu().numpy())
    for l, tau in enumerate(lags):
        alone = eng.tica_moments(x, off, lags[l:l + 1], 1)
        for a, b in zip(ref, alone):
            assert np.array_equal(a[l], b[0]), int(tau)
    wide = np.full((len(x), 24, 3), np.nan, np.float32)
    wide[:, 2:, 2] = x
    for got in (eng.tica_moments(wide[:, 2:, 2], off, lags, 1), eng.tica_moments(torch.as_tensor(wide).cuda()[:, 2:, 2], off, lags, 1)):
        for a, b in zip(ref, got):
            assert np.array_equal(a, b.cpu().numpy() if hasattr(b, "data_ptr") else b)


@pytest.mark.parametrize("K", [2, 8, 22, 32])
def test_fit_against_the_restatement(eng, K):
    """The algebra alone: the device is fed the restatement's moments.  Ranks exact; eigenvalues within 64 max(ev_dev, d 2^-52), ev_dev
    the deviation of the two LAPACK routes on the same moments; component k within that allowance times ||R_k|| / gap_k, on inputs
    where the two CPU routes stay below a third of that bar; the sign rule exactly; scaling 0 against 1 differs by lambda_k exactly."""
    x, off, _ = tn.synthetic(K, LENGTHS, seed=K)
    count, sm, cov = tn.moments(x, off, LAGS)
    d, dim = 2 * K, min(4, 2 * K)
    mean, ev, comp, rank = eng.tica_fit(count, sm, cov, dim, 1e-6, 1)
    _, ev0, comp0, _ = eng.tica_fit(count, sm, cov, dim, 1e-6, 0)
    assert mean.shape == (3, d) and ev.shape == (3, dim) and comp.shape == (3, d, dim) and rank.dtype == np.int32
    assert np.array_equal(ev, ev0) and np.array_equal(comp, comp0 * ev[:, None, :])
    for l in range(len(LAGS)):
        mu, rev, R, r = tn.fit(count[l], sm[l], cov[l], dim)
        _, gev, G, _ = tn.fit_generalized(count[l], sm[l], cov[l], dim)
        lam = tn.fit(count[l], sm[l], cov[l], d)[1]
        ev_dev = np.abs(rev - gev).max()
        allow = 64 * max(ev_dev, d * 2.0 ** -52)
        assert rank[l] == r == d
        np.testing.assert_allclose(mean[l], mu, rtol=0, atol=4 * 2.0 ** -53)
        print(f"K={K} lag={LAGS[l]}: eigenvalues off by {np.abs(ev[l] - rev).max():.2e} (allowed {allow:.2e}, ev_dev {ev_dev:.2e})")
        assert np.abs(ev[l] - rev).max() <= allow
        for k in range(dim):
            gap = np.abs(np.delete(lam, k) - lam[k]).min()
            bar = allow * np.linalg.norm(R[:, k]) / gap
            assert np.linalg.norm(R[:, k] - G[:, k]) <= bar / 3
            print(f"    component {k}: off by {np.linalg.norm(comp[l, :, k] - R[:, k]):.2e} (allowed {bar:.2e})")
            assert np.linalg.norm(comp[l, :, k] - R[:, k]) <= bar
            f = int(np.argmax(np.abs(comp0[l, :, k])))
            assert comp0[l, f, k] > 0


def test_fit_rank_deficient(eng):
    """encode = 0 with one duplicated and one constant column: rank d - 2, NaN beyond it (no C00 eigenvalue lies within a factor 1e3 of
    epsilon: tests/test_tica_host.py checks that on the CPU).  The kept eigenvalues, the mean and the kept components against the
    restatement on the restatement's moments, under the bar of the full-rank test with its floor d 2^-52 as the allowance (the second
    LAPACK route needs full rank); then the device's own moments give the same rank and pattern."""
    x, off = deficient_set()
    d = 5
    rcount, rsm, rcov = tn.moments(x, off, [2], enc=False)
    rmu, rev, R, r = tn.fit(rcount[0], rsm[0], rcov[0], d)
    mean, ev, comp, rank = eng.tica_fit(rcount, rsm, rcov, d, 1e-6, 1)
    assert rank[0] == r == 3
    assert np.all(np.isfinite(ev[0, :3])) and np.all(np.isnan(ev[0, 3:])) and np.all(np.isfinite(comp[0, :, :3])) and np.all(np.isnan(comp[0, :, 3:]))
    allow = 64 * d * 2.0 ** -52
    assert np.abs(ev[0, :3] - rev[:3]).max() <= allow
    np.testing.assert_allclose(mean[0], rmu, rtol=0, atol=4 * 2.0 ** -53 * np.abs(rmu).max())
    for k in range(3):
        gap = np.abs(np.delete(rev[:3], k) - rev[k]).min()
        bar = allow * np.linalg.norm(R[:, k]) / gap
        print(f"rank-deficient component {k}: off by {np.linalg.norm(comp[0, :, k] - R[:, k]):.2e} (allowed {bar:.2e})")
        assert np.linalg.norm(comp[0, :, k] - R[:, k]) <= bar
    count, sm, cov = eng.tica_moments(x, off, np.array([2], np.int32), 0)
    mean, ev, comp, rank = eng.tica_fit(count, sm, cov, d, 1e-6, 1)
    assert rank[0] == 3 and np.all(np.isfinite(comp[0, :, :3])) and np.all(np.isnan(comp[0, :, 3:])) and np.all(np.isnan(ev[0, 3:]))
    y = eng.tica_transform(x, mean, comp, 0)
    assert y.shape == (1, len(x), 5) and np.all(np.isfinite(y[0, :, :3])) and np.all(np.isnan(y[0, :, 3:]))


@pytest.mark.parametrize("K,enc", [(1, 0), (3, 1), (22, 1), (32, 0), (32, 1)])
def test_transform_against_the_restatement(eng, K, enc):
    """Within one fp32 ulp of the value plus the fp64 sum bound (``transform_bound``); a NaN row stays a NaN row and its neighbours
    are untouched; more than one block of rows; strided values give the bits of a contiguous copy."""
    x, off, _ = tn.synthetic(K, [700, 333], seed=40 + K)
    d = 2 * K if enc else K
    dim = min(3, d)
    count, sm, cov = tn.moments(x, off, [1, 5], enc)
    model = [tn.fit(count[l], sm[l], cov[l], dim) for l in range(2)]
    mean, comp = np.stack([m[0] for m in model]), np.stack([m[2] for m in model])
    y = eng.tica_transform(x, mean, comp, enc)
    assert y.shape == (2, len(x), dim) and y.dtype == np.float32
    for l in range(2):
        ref = tn.transform(x, mean[l], comp[l], enc)
        tol = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) + tn.transform_bound(x, mean[l], comp[l], enc)
        assert np.all(np.abs(y[l] - ref) <= tol), np.max(np.abs(y[l] - ref) / tol)
    xb = x.copy()
    xb[5, K // 2], xb[300, 0] = np.nan, np.inf
    yb = eng.tica_transform(xb, mean, comp, enc)
    assert np.all(np.isnan(yb[:, [5, 300]]))
    keep = np.ones(len(x), bool)
    keep[[5, 300]] = False
    assert np.array_equal(yb[:, keep], y[:, keep])
    wide = np.full((len(x), K + 2, 3), np.nan, np.float32)
    wide[:, 2:, 2] = x
    import torch
    yd = eng.tica_transform(torch.as_tensor(wide).cuda()[:, 2:, 2], torch.as_tensor(mean).cuda(), torch.as_tensor(comp).cuda(), enc)
    assert yd.is_cuda and np.array_equal(yd.cpu().numpy(), y)


def test_end_to_end_recovers_the_slow_column(eng):
    """observables.tica_fit + tica_marginals on the K = 2 synthetic set: tIC 1 follows the well index of the slowest torsion (|corr| above
    0.9; the restatement gives 0.954 and 0.957 at these lags, tests/test_tica_host.py).  On device tensors too: the same bits."""
    import torch
    obs = pkg().observables
    x, off, wells = tn.synthetic(2, LENGTHS, seed=0)
    m = obs.tica_fit(x, off, [64, 128], engine=eng)
    assert m.lags.tolist() == [64, 128] and m.rank.tolist() == [4, 4] and m.components.shape == (2, 4, 2) and m.timescales.shape == (2, 2)
    np.testing.assert_allclose(m.timescales, -np.array([[64.0], [128.0]]) / np.log(m.eigenvalues))
    y = obs.tica_transform(m, x, engine=eng)
    for l in range(2):
        corr = np.corrcoef(y[l, :, 0], wells[:, 0])[0, 1]
        print(f"lag {m.lags[l]}: corr(tIC 1, slow well) = {corr:.4f}, eigenvalues {m.eigenvalues[l]}")
        assert abs(corr) > 0.9
    mg = obs.tica_marginals(m, x, engine=eng)
    assert mg.hist.shape == (2, 2, 80) and mg.tails.shape == (2, 2, 3) and mg.edges.shape == (81,)
    np.testing.assert_allclose(mg.hist.sum(axis=2) + mg.tails.sum(axis=2), 1.0, atol=1e-12)
    for l in range(2):
        for k in range(2):
            h, _ = np.histogram(y[l, :, k].astype(np.float64), bins=80, range=(-2.5, 2.5))
            assert np.abs(mg.hist[l, k] - h / len(x)).max() <= 2.0 / len(x)      # a value on an edge may fall either way in numpy
    md = obs.tica_fit(torch.as_tensor(x).cuda(), off, [64, 128], engine=eng)
    assert md.components.is_cuda and np.array_equal(md.components.cpu().numpy(), m.components) and np.array_equal(md.timescales, m.timescales)
    logw = np.linspace(-1.0, 1.0, len(x)).astype(np.float32)
    mw = obs.tica_marginals(m, x, logw=logw, keep=(np.arange(len(x)) % 3 > 0).astype(np.uint8), engine=eng)
    np.testing.assert_allclose(mw.hist.sum(axis=2) + mw.tails.sum(axis=2), 1.0, atol=1e-12)


def test_refusals_leave_the_outputs_untouched(eng):
    ti = pkg()
    L, lib = ti._lib.lib(), ti._lib
    p = lambda a: C.c_void_p(a.ctypes.data)
    x, off, _ = tn.synthetic(3, [40, 25], seed=3)
    lags = np.array([1, 2], np.int32)

    def mom(x=x, n=None, off=off, lags=lags, K=3):
        count, sm, cov = np.full(len(lags), -7, np.int64), np.full((len(lags), 2, 2 * K), -7.0), np.full((len(lags), 3, 2 * K, 2 * K), -7.0)
        rc = L.ti_obs_tica_moments(eng.h, p(x), K, 1, len(x) if n is None else n, K, 1, off.ctypes.data_as(C.POINTER(C.c_int64)), len(off) - 1,
                                   lib.iptr(lags), len(lags), p(count), p(sm), p(cov), lib.MEM_HOST)
        return rc, lib.last_error(), all(np.all(a == -7) for a in (count, sm, cov))

    rc, _, untouched = mom()
    assert rc == lib.TI_OK and not untouched
    xb = x.copy()
    xb[44, 1], xb[50, 0] = np.inf, np.nan
    rc, msg, untouched = mom(x=xb)
    assert rc == lib.TI_E_NAN and "row 44" in msg and untouched                # found on the device, the first row named
    rc, msg, untouched = mom(lags=np.array([1, 39], np.int32))
    assert rc == lib.TI_E_ARG and "lag 39" in msg and untouched                # one pair
    big = (1 << 27) // 16 + 1
    rc, msg, untouched = mom(n=big, off=np.array([0, big], np.int64))
    assert rc == lib.TI_E_ALLOC and untouched                                  # refused before the values are read
    with pytest.raises(lib.TiError):
        eng.tica_moments(xb, off, lags, 1)

    count, sm, cov = tn.moments(x, off, lags)

    def fit(count=count, sm=sm, cov=cov, dim=2):
        desc = lib.TicaDesc(dim, 1, 0, 1e-6)
        out = [np.full((2, 6), -7.0), np.full((2, dim), -7.0), np.full((2, 6, dim), -7.0), np.full(2, -7, np.int32)]
        rc = L.ti_obs_tica_fit(eng.h, p(count), p(sm), p(cov), 2, 6, C.byref(desc), *(p(a) for a in out), lib.MEM_HOST)
        return rc, lib.last_error(), all(np.all(a == -7) for a in out)

    rc, _, untouched = fit()
    assert rc == lib.TI_OK and not untouched
    c1 = count.copy()
    c1[1] = 1
    rc, msg, untouched = fit(count=c1)
    assert rc == lib.TI_E_ARG and "count 1" in msg and untouched
    for which in (1, 2):
        arrs = [count, sm.copy(), cov.copy()]
        arrs[which].reshape(-1)[-1] = np.nan
        rc, msg, untouched = fit(*arrs)
        assert rc == lib.TI_E_NAN and "lag entry 1" in msg and untouched
