"""ti_obs_rff_gram_wide on the GPU: the blocked Gram pass (128 < p <= 1024) against the numpy restatement (tests/gedmd_numpy.py) within
the derived bound of tests/test_gpu_gedmd.py (gedmd_numpy.gram_bound), exact Hermitian symmetry, determinism bit for bit (repeat,
generator against explicit rows, addressing of global resamples, the two memory modes, rows per launch, p <= 128 against
ti_obs_rff_gram, and the 16 x 16 tiles of a wide result against the narrow call on those column tiles), the refusals found on the
device, and the reference's eigenvalues and cross-validated scores end to end (tests/golden/gedmd_wide_reference.npz)."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg
import boot_numpy as bn
from test_gedmd_wide_host import fixture_cases
from test_gpu_gedmd import S, check_rows, data, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    return pkg().observables._service_engine(0)


# (n, d, p, logw): every p in {129, 144, 256, 257, 300, 1024} (one tile past a panel, a one-tile and a full last panel, a padded last
# tile, the study's size, the cap), d in {1, 6, 16}, n in {1, 5, 65, S + 1 (two segments)}, with and without weights
CASES = [(1, 1, 129, False), (65, 1, 129, True), (5, 6, 144, True), (S + 1, 6, 144, False), (65, 16, 256, False), (S + 1, 1, 257, True),
         (5, 1, 300, True), (S + 1, 6, 300, False), (1, 16, 1024, True), (65, 6, 1024, True), (S + 1, 16, 1024, False)]


@pytest.mark.parametrize("n,d,p,weighted", CASES)
def test_wide_gram_against_the_restatement(eng, n, d, p, weighted):
    """Host memory: the point estimate and two generator rows (first + r crosses 2^32); the same rows through indices give the same bits."""
    x, logw = data(n, d, 1000 * p + n, weighted)
    omega = np.random.RandomState(p).randn(d, p) / (0.6 if d == 1 else 2.0)
    seed, first = 0x9E3779B97F4A7C15, 2 ** 32 - 1
    G = eng.rff_gram_wide(x, omega, logw, 2, first, seed)
    rows = bn.draw_rows(seed, first, 2, n, n)
    worst = [0.0]
    check_rows(G, x, omega, logw, [None, *rows], worst, f"n{n}-d{d}-p{p}")
    assert same_bits(G, eng.rff_gram_wide(x, omega, logw, 2, indices=rows))
    print(f"worst fraction of the bound {worst[0]:.3f}")


def test_rows_do_not_depend_on_the_call(eng):
    """p = 300, two segments: a repeat call; n_boot = 3 against rows 0..2 of n_boot = 7; row R of first = 0 is row 0 of first = R; device
    memory against host memory."""
    import torch
    n, d, p = S + 1, 6, 300
    x, logw = data(n, d, 21, True)
    omega = np.random.RandomState(6).randn(d, p) / 2.0
    G = eng.rff_gram_wide(x, omega, logw, 7, 0, 42)
    assert same_bits(G, eng.rff_gram_wide(x, omega, logw, 7, 0, 42))
    assert same_bits(G[:4], eng.rff_gram_wide(x, omega, logw, 3, 0, 42))
    for R in (3, 6):
        one = eng.rff_gram_wide(x, omega, logw, 1, R, 42)
        assert same_bits(one[1], G[1 + R]) and same_bits(one[0], G[0])
    Gd = eng.rff_gram_wide(torch.from_numpy(x).cuda(), omega, torch.from_numpy(logw).cuda(), 7, 0, 42)
    assert Gd.is_cuda and same_bits(Gd, G)
    assert not same_bits(G[1], G[2]) and not same_bits(G[1], eng.rff_gram_wide(x, omega, logw, 1, 0, 43)[1])


def test_rows_do_not_depend_on_the_rows_per_launch(eng):
    """p = 1024 (2080 tiles of 4 KB a row and segment): 31 rows fill the 256 MiB of partial tiles of a launch, so 40 rows take two
    launches; the rows on both sides of the cut are those of single-row calls."""
    import torch
    n, d, p, nb = 65, 6, 1024, 40
    x, _ = data(n, d, 33, False)
    omega = np.random.RandomState(7).randn(d, p) / 2.0
    xd = torch.from_numpy(x).cuda()
    G = eng.rff_gram_wide(xd, omega, None, nb, 0, 5)
    for R in (0, 30, 31, 39):
        assert same_bits(eng.rff_gram_wide(xd, omega, None, 1, R, 5)[1], G[1 + R]), R
    check_rows(G[[0, 32]], x, omega, None, [None, bn.draws(5, 31, n, n)], [0.0], "two launches")


@pytest.mark.parametrize("p", [50, 128])
def test_narrow_sizes_through_the_wide_entry_are_the_narrow_call(eng, p):
    n, d = S + 1, 3
    x, logw = data(n, d, p, True)
    omega = np.random.RandomState(p).randn(d, p) / 0.6
    assert same_bits(eng.rff_gram_wide(x, omega, logw, 2, 1, 9), eng.rff_gram(x, omega, logw, 2, 1, 9))


def test_a_tile_of_the_wide_result_is_the_narrow_result_of_its_column_tiles(eng):
    """p = 300 in 19 column tiles (panels of 8, 8 and 3; the last tile padded), two segments: the sub-blocks of column tiles {0, 9, 18}
    -- a diagonal pair of each panel and the three off-diagonal pairs between them -- hold the bits ti_obs_rff_gram gives for omega
    restricted to those columns (three tiles, the last padded alike).  No tolerance: this pins the panel and tile index arithmetic."""
    n, d, p = S + 1, 6, 300
    x, logw = data(n, d, 99, True)
    omega = np.random.RandomState(12).randn(d, p) / 2.0
    cols = np.concatenate([np.arange(16 * t, min(16 * t + 16, p)) for t in (0, 9, 18)])
    assert cols.size == 44
    G = eng.rff_gram_wide(x, omega, logw, 2, 0, 3)
    Gn = eng.rff_gram(x, np.ascontiguousarray(omega[:, cols]), logw, 2, 0, 3)
    assert same_bits(np.ascontiguousarray(G[:, cols][:, :, cols]), Gn)
    # and every other choice of three tiles that fits a quick test: one per panel pair class, through the point estimate alone
    for tiles in ((7, 8, 16), (1, 15, 17), (8, 17, 18)):
        cols = np.concatenate([np.arange(16 * t, min(16 * t + 16, p)) for t in tiles])
        assert same_bits(np.ascontiguousarray(G[:1, cols][:, :, cols]), eng.rff_gram(x, np.ascontiguousarray(omega[:, cols]), logw)), tiles


def test_refusals_found_on_the_device(eng):
    ti = pkg()
    n, d, p = 65, 2, 144
    x, logw = data(n, d, 3, True)
    omega = np.random.RandomState(2).randn(d, p) / 0.6
    g = ti._lib.GramDesc(d, p, 2, 0, 0)
    out = np.full((3, p, p, 2), 7.0)
    for bad in (n, -1, 2 ** 31 - 1):
        idx = np.zeros((2, 10), np.int32)
        idx[1, 9] = bad
        rc = ti._lib.lib().ti_obs_rff_gram_wide(eng.h, C.c_void_p(x.ctypes.data), d, n, omega.ctypes.data_as(C.POINTER(C.c_double)),
                                                C.c_void_p(logw.ctypes.data), C.byref(g), C.c_void_p(idx.ctypes.data), 10, C.c_void_p(out.ctypes.data), 0)
        assert rc == ti._lib.TI_E_ARG and f"idx entry outside 0..{n - 1}" in ti._lib.last_error()
        assert (out == 7.0).all()
    lw = logw.copy()
    lw[41] = np.nan
    with pytest.raises(ti._lib.TiError, match="non-finite logw at index 41") as e:
        eng.rff_gram_wide(x, omega, lw, 2)
    assert e.value.code == ti._lib.TI_E_NAN
    # the handle works on
    check_rows(eng.rff_gram_wide(x, omega, logw), x, omega, logw, [None], [0.0], "after the refusals")


def test_fixture_rows_and_splits_reproduce_the_reference(eng):
    """gedmd_generator with the reference's own index rows (p = 300 twice, 513, and the narrower cases) and gedmd_cv with its recorded
    splits: eigenvalues within 64 ev_dev, scores within 64 score_dev (the allowance of tests/test_gpu_gedmd.py), ranks exactly."""
    obs = pkg().observables
    cases, ev_dev, score_dev = fixture_cases()
    worst = [0.0, 0.0]
    for c in cases:
        res = obs.gedmd_generator(c["x"], c["omega"], c["nev"], c["a"], tol=c["tol"], n_boot=3, indices=c["idx"], engine=eng)
        got = np.concatenate([res.eigenvalues[None], res.estimates])
        cv = obs.gedmd_cv(c["x"], c["omega"], c["a"], c["nev"], c["tol"], rtrain=c["rtrain"], splits=c["perm"], engine=eng)
        dev = (max(np.abs(got - c["ev"]).max(), np.abs(cv.eigenvalues - c["cv_ev"]).max()), np.abs(cv.scores - c["cv_score"]).max())
        print(f"{c['name']}: eigenvalues {dev[0]:.2e} (64 ev_dev = {64 * ev_dev:.2e}), scores {dev[1]:.2e} (64 score_dev = {64 * score_dev:.2e})")
        worst = [max(worst[0], dev[0]), max(worst[1], dev[1])]
        assert res.rank == c["rank"][0] and res.eigenvectors.shape == (c["p"], c["nev"])
        np.testing.assert_array_equal(cv.rank, c["cv_rank"])
        assert dev[0] <= 64 * ev_dev and dev[1] <= 64 * score_dev, (c["name"], dev)
    print(f"GPU against the reference: worst eigenvalue difference {worst[0]:.2e}, worst score difference {worst[1]:.2e}")


def test_cv_on_device_tensors_is_cv_on_host_arrays(eng):
    import torch
    obs = pkg().observables
    x, _ = data(600, 2, 8, False)
    omega = obs.sample_rff_gaussian(2, 130, 0.8, 1)
    host = obs.gedmd_cv(x, omega, 1.6, 3, 1e-4, ntest=4, seed=2, engine=eng)
    dev = obs.gedmd_cv(torch.from_numpy(x).cuda(), omega, 1.6, 3, 1e-4, ntest=4, seed=2, engine=eng)
    np.testing.assert_array_equal(host.eigenvalues, dev.eigenvalues)
    np.testing.assert_array_equal(host.scores, dev.scores)
    assert host.scores.shape == (4,) and np.isfinite(host.scores).all()
