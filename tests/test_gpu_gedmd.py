"""ti_obs_rff_gram on the GPU: the Gram matrices against their numpy restatement (tests/gedmd_numpy.py) at the sizes where tiling,
padding and segmenting can go wrong, exact Hermitian symmetry, weights as multiplicities, determinism (generator against explicit
rows, addressing of global resamples, the two memory modes, rows per launch), the reference's eigenvalues end to end through explicit
index rows (tests/golden/gedmd_reference.npz), a statistical check of the generator path, and the refusals found on the device.

Entrywise bound on a row's Gram matrix, real and imaginary part each: 2 W (4 n_draw + 2 (d + 1) Phi + 8) 2^-53 (gedmd_numpy.gram_bound:
a fixed-order sum of 2 n_draw terms of magnitude <= 1, the rounding of the phase, two <= 2-ulp sincos; the outer 2 because the oracle
errs too).  Worst observed fraction of it over every row checked here, MI355X: 0.062 (n = 2, p = 15; 0.002 at n >= 4097); the recorded
reference eigenvalues are met to 5.5e-11 (allowed 64 ev_dev = 1.5e-9)."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg
import boot_numpy as bn
import gedmd_numpy as gn
from test_gedmd_host import fixture_cases

pytestmark = pytest.mark.gpu
S = 8192                      # GRAM_SEG of csrc/ti_internal.hpp: draws per (row, segment) workgroup


@pytest.fixture(scope="module")
def eng():
    return pkg().observables._service_engine(0)


def data(n, d, seed, logw):
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((n, d))
    x[:, 0] = np.where(rs.random_sample(n) < 0.5, -1.0, 1.0) + 0.35 * x[:, 0]
    return x.astype(np.float32), (rs.standard_normal(n) * 2.0).astype(np.float32) if logw else None


def same_bits(a, b):
    a, b = (np.ascontiguousarray(v.detach().cpu().numpy() if hasattr(v, "data_ptr") else v, np.complex128) for v in (a, b))
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_rows(G, x, omega, logw, rows, worst, what):
    """every row of G against the oracle within the bound; exactly Hermitian, Im of the diagonal 0"""
    G = np.asarray(G.detach().cpu().numpy() if hasattr(G, "data_ptr") else G)
    assert G.shape == (len(rows), omega.shape[1], omega.shape[1]) and G.dtype == np.complex128
    for g, row in zip(G, rows):
        ref, b = gn.gram(x, omega, row, logw), gn.gram_bound(x, omega, row, logw)
        err = max(np.abs(g.real - ref.real).max(), np.abs(g.imag - ref.imag).max())
        worst[0] = max(worst[0], err / b)
        print(f"{what}: n_draw {x.shape[0] if row is None else len(row)} error {err:.3e} bound {b:.3e} fraction {err / b:.3f}")
        assert err <= b, (what, err, b)
        assert np.array_equal(g.real, g.real.T) and np.array_equal(g.imag, -g.imag.T) and (g.imag.diagonal() == 0).all(), what


# (n, d, p, logw): every p in {1, 15, 16, 17, 50, 128}, d in {1, 3, 16}, n in {1..5, 63, 64, 65, 257, 4097, S - 1, S, S + 1, 2 S + 1}
CASES = [(1, 1, 1, False), (2, 1, 15, True), (3, 3, 16, False), (4, 1, 17, True), (5, 16, 50, False), (63, 1, 128, True), (64, 3, 17, True),
         (65, 1, 50, False), (257, 16, 16, True), (4097, 1, 50, True), (S - 1, 1, 17, False), (S, 3, 15, True), (S + 1, 1, 128, True),
         (2 * S + 1, 1, 50, False), (2 * S + 1, 16, 1, True)]


@pytest.mark.parametrize("n,d,p,weighted", CASES)
def test_gram_against_the_restatement(eng, n, d, p, weighted):
    """Host memory: the point estimate and two generator rows (first + r crosses 2^32); the same rows through indices give the same bits."""
    x, logw = data(n, d, 1000 * p + n, weighted)
    omega = np.random.RandomState(p).randn(d, p) / 0.6
    seed, first = 0x9E3779B97F4A7C15, 2 ** 32 - 1
    G = eng.rff_gram(x, omega, logw, 2, first, seed)
    rows = bn.draw_rows(seed, first, 2, n, n)
    worst = [0.0]
    check_rows(G, x, omega, logw, [None, *rows], worst, f"n{n}-d{d}-p{p}")
    assert same_bits(G, eng.rff_gram(x, omega, logw, 2, indices=rows))
    print(f"worst fraction of the bound {worst[0]:.3f}")


def test_strided_values_on_the_device_and_a_draw_count_of_its_own(eng):
    """A column view of a wider array (stride > d) read in place on the device, and n_draw != n through indices."""
    import torch
    n, d, p = 65, 3, 17
    x, logw = data(n, d, 5, True)
    omega = np.random.RandomState(3).randn(d, p) / 0.6
    wide = np.full((n, 5), np.nan, np.float32)                       # the columns beyond d are never read
    wide[:, :d] = x
    rows = np.random.RandomState(8).randint(0, n, (3, 100)).astype(np.int32)
    Gd = eng.rff_gram(torch.from_numpy(wide).cuda()[:, :d], omega, torch.from_numpy(logw).cuda(), 3, indices=torch.from_numpy(rows).cuda())
    assert Gd.is_cuda and Gd.dtype == torch.complex128
    check_rows(Gd, x, omega, logw, [None, *rows], [0.0], "strided")
    assert same_bits(Gd, eng.rff_gram(x, omega, logw, 3, indices=rows))              # host memory: the same bits
    # the C entry point with a host stride > d
    ti = pkg()
    out = np.empty((1, p, p, 2))
    g = ti._lib.GramDesc(d, p, 0, 0, 0)
    ti._lib.check(ti._lib.lib().ti_obs_rff_gram(eng.h, C.c_void_p(wide.ctypes.data), 5, n, omega.ctypes.data_as(C.POINTER(C.c_double)),
                                               C.c_void_p(logw.ctypes.data), C.byref(g), None, 0, C.c_void_p(out.ctypes.data), 0))
    assert same_bits(out.view(np.complex128)[..., 0], Gd[:1])


def test_integer_weights_are_multiplicities(eng):
    """logw = ln c_n: the Gram matrix of the explicit row that repeats sample n c_n times, scaled by 1 / max c.  The fp32 rounding of
    ln c is an input error the bound of the contraction does not know: the weights the inputs define are exp(fp32(ln c_n) - fp32(ln
    max c)), not c_n / max c, and every term of an entry is at most w_n in magnitude, so the sum of those differences (computed from
    the inputs, 3.4e-6 here; observed difference 1.2e-6) is added to the two rows' bounds."""
    n, d, p = 257, 1, 50
    x, _ = data(n, d, 77, False)
    omega = np.random.RandomState(4).randn(d, p) / 0.6
    c = np.random.RandomState(5).randint(1, 8, n)
    c[0] = 8
    row = np.repeat(np.arange(n), c).astype(np.int32)
    lw = np.log(c).astype(np.float32)
    Gw = eng.rff_gram(x, omega, lw)[0]
    Gr = eng.rff_gram(x, omega, None, 1, indices=row[None])[1] / 8.0
    b = gn.gram_bound(x, omega, row) / 8.0 + gn.gram_bound(x, omega, None, lw) + np.abs(gn.weights(lw) - c / 8.0).sum()
    err = max(np.abs(Gw.real - Gr.real).max(), np.abs(Gw.imag - Gr.imag).max())
    print(f"multiplicities: error {err:.3e} bound {b:.3e}")
    assert err <= b
    # and against the oracle with the very weights the library forms: the contraction's own bound
    check_rows(Gw[None], x, omega, lw, [None], [0.0], "weighted")


def test_rows_do_not_depend_on_the_call(eng):
    """Row R of (first, n_boot) = (0, 8) is row 0 of (R, 1); a repeat call and device memory give the same bits."""
    import torch
    n, d, p = S + 1, 1, 17
    x, logw = data(n, d, 21, True)
    omega = np.random.RandomState(6).randn(d, p) / 0.6
    G = eng.rff_gram(x, omega, logw, 8, 0, 42)
    assert same_bits(G, eng.rff_gram(x, omega, logw, 8, 0, 42))
    for R in (0, 3, 7):
        one = eng.rff_gram(x, omega, logw, 1, R, 42)
        assert same_bits(one[1], G[1 + R]) and same_bits(one[0], G[0])
    Gd = eng.rff_gram(torch.from_numpy(x).cuda(), omega, torch.from_numpy(logw).cuda(), 8, 0, 42)
    assert same_bits(Gd, G)
    assert not same_bits(G[1], G[2]) and not same_bits(G[1], eng.rff_gram(x, omega, logw, 1, 0, 43)[1])


def test_rows_do_not_depend_on_the_rows_per_launch(eng):
    """p = 128 (36 tiles) and two segments: 910 rows fill the 256 MiB of partial tiles of a launch, so 912 rows take two launches; the
    rows on both sides of the cut are those of single-row calls."""
    import torch
    n, d, p, nb = S + 1, 1, 128, 912
    x, _ = data(n, d, 33, False)
    omega = np.random.RandomState(7).randn(d, p) / 0.6
    xd = torch.from_numpy(x).cuda()
    G = eng.rff_gram(xd, omega, None, nb, 0, 5)
    for R in (0, 909, 910, 911):
        assert same_bits(eng.rff_gram(xd, omega, None, 1, R, 5)[1], G[1 + R]), R
    check_rows(G[[0, 911]], x, omega, None, [None, bn.draws(5, 910, n, n)], [0.0], "two launches")


def test_fixture_rows_reproduce_the_reference(eng):
    """gedmd_generator with the reference's own index rows: its eigenvalues within 64 ev_dev, its ranks exactly."""
    obs = pkg().observables
    cases, ev_dev = fixture_cases()
    worst = 0.0
    for c in cases:
        res = obs.gedmd_generator(c["x"], c["omega"], c["nev"], c["a"], tol=c["tol"], n_boot=3, indices=c["idx"], engine=eng)
        got = np.concatenate([res.eigenvalues[None], res.estimates])
        worst = max(worst, np.abs(got - c["ev"]).max())
        assert np.abs(got - c["ev"]).max() <= 64 * ev_dev, (c["name"], np.abs(got - c["ev"]).max())
        assert res.rank == c["rank"][0] and res.eigenvectors.shape == (c["p"], c["nev"]) and res.ci.shape == (2, c["nev"])
        _, _, r = obs.gedmd_spectrum(obs.rff_gram(c["x"], c["omega"], n_boot=3, indices=c["idx"], engine=eng), c["omega"], c["a"], c["nev"], c["tol"])
        np.testing.assert_array_equal(r, c["rank"])
    print(f"GPU against the reference: worst eigenvalue difference {worst:.2e} (64 ev_dev = {64 * ev_dev:.2e})")


def test_generator_path_statistics(eng):
    """n = 4096, 400 resamples: the mean of the second-slowest eigenvalue's estimates within 4 of their standard errors of the point
    estimate; the interval brackets the point estimate."""
    obs = pkg().observables
    x, _ = data(4096, 1, 2024, False)
    omega = obs.sample_rff_gaussian(1, 50, 0.6, 1)
    res = obs.gedmd_generator(x, omega, 4, 1.6, tol=1e-4, n_boot=400, seed=7, engine=eng)
    est = res.estimates[:, -2]
    se = est.std(ddof=1) / np.sqrt(est.size)
    print(f"point {res.eigenvalues[-2]:.5f} mean {est.mean():.5f} std {est.std(ddof=1):.5f} se {se:.5f} -> {(est.mean() - res.eigenvalues[-2]) / se:.2f} se")
    assert abs(est.mean() - res.eigenvalues[-2]) <= 4 * se
    assert res.ci[0, -2] < res.eigenvalues[-2] < res.ci[1, -2] and res.estimates.shape == (400, 4)
    assert abs(res.eigenvalues[-1]) < 1e-6                         # the constant function


def test_refusals_found_on_the_device(eng):
    ti = pkg()
    n, d, p = 65, 1, 8
    x, logw = data(n, d, 3, True)
    omega = np.random.RandomState(2).randn(d, p) / 0.6
    g = ti._lib.GramDesc(d, p, 2, 0, 0)
    out = np.full((3, p, p, 2), 7.0)
    for bad in (n, -1, 2 ** 31 - 1):
        idx = np.zeros((2, 10), np.int32)
        idx[1, 9] = bad
        rc = ti._lib.lib().ti_obs_rff_gram(eng.h, C.c_void_p(x.ctypes.data), d, n, omega.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(logw.ctypes.data),
                                           C.byref(g), C.c_void_p(idx.ctypes.data), 10, C.c_void_p(out.ctypes.data), 0)
        assert rc == ti._lib.TI_E_ARG and f"idx entry outside 0..{n - 1}" in ti._lib.last_error()
        assert (out == 7.0).all()
    lw = logw.copy()
    lw[41] = np.nan
    with pytest.raises(ti._lib.TiError, match="non-finite logw at index 41") as e:
        eng.rff_gram(x, omega, lw, 2)
    assert e.value.code == ti._lib.TI_E_NAN
    # the handle works on
    check_rows(eng.rff_gram(x, omega, logw), x, omega, logw, [None], [0.0], "after the refusals")
