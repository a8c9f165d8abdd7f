"""ti_obs_bootstrap on the GPU: the reference's own bootstrap replayed through explicit index rows (tests/golden/boot_reference.npz),
the generator pinned to its numpy restatement (tests/boot_numpy.py), determinism, the addressing of global resamples, the two memory
modes, the Python wrappers, a statistical check of the generator, and the refusals that are found on the device.

Worst error against the reference over the whole fixture, MI355X: 0.095 of the bound 8 n_draw 2^-53 (1 + |ref|)."""
import numpy as np
import pytest

from conftest import pkg
import boot_numpy as bn
from test_boot_host import check_against_fixture, fixture_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    return pkg().observables._service_engine(0)


def run(eng, logw, estimator, mode=bn.NONE, k=1.5, n_boot=8, first=0, seed=0, indices=None, level=0.95):
    return eng.bootstrap(logw, estimator, mode, k, level, n_boot, first, seed, indices)


def sample(n, seed=1, sd=3.0):
    return (np.random.RandomState(seed).standard_normal(n) * sd).astype(np.float32)


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


def test_explicit_rows_reproduce_the_reference(eng):
    worst = [0.0]
    for c in fixture_cases():
        point, lo, hi, kept, est = run(eng, c["logw"], c["estimator"], c["mode"], c["k"], c["n_boot"], indices=c["idx"] if c["n_draw"] else None)
        check_against_fixture(c, point, lo, hi, kept, est, worst)
    print(f"GPU against the reference: worst error {worst[0]:.3f} of the bound")


CONFIGS = [(257, bn.ESS, bn.ONCE, 1.5, 0), (1000, bn.TFEP, bn.RESAMPLE, 100.0, 0), (65, bn.MEAN, bn.NONE, 1.5, 0), (4097, bn.TFEP, bn.RESAMPLE, 1.5, 777),
           (600, bn.MEAN, bn.RESAMPLE, 1.5, 513), (3, bn.ESS, bn.NONE, 1.5, 1), (1, bn.TFEP, bn.NONE, 1.5, 0)]


@pytest.mark.parametrize("n,estimator,mode,k,n_draw", CONFIGS)
def test_generator_equals_its_restatement(eng, n, estimator, mode, k, n_draw):
    """The generator's rows are the restated rows: a call on those rows through idx gives the same bits, and the numpy bootstrap on
    the restated rows gives the same numbers to the fixture's bound."""
    logw, seed, first, nb = sample(n, seed=n), 0x9E3779B97F4A7C15, 2 ** 32 - 2, 5              # first + r crosses the counter's word boundary
    n_pop = run(eng, logw, estimator, mode, k, 0)[3] if mode == bn.ONCE else n
    nd = n_draw or n_pop
    rows = bn.draw_rows(seed, first, nb, nd, n_pop)
    if n_draw:                                       # n_draw != 0 goes through the engine only with rows; call the library for the generator
        import ctypes as C
        ti = pkg()
        d = ti._lib.BootDesc(estimator, mode, k, 0.95, nb, first, seed)
        out, gen_est = (C.c_double * 4)(), np.empty(nb)
        ti._lib.check(ti._lib.lib().ti_obs_bootstrap(eng.h, C.c_void_p(logw.ctypes.data), n, C.byref(d), None, nd, out, C.c_void_p(gen_est.ctypes.data), 0))
        gen = (out[0], out[1], out[2], int(out[3]), gen_est)
    else:
        gen = run(eng, logw, estimator, mode, k, nb, first, seed)
    exp = run(eng, logw, estimator, mode, k, nb, indices=rows)
    assert same_bits(gen[4], exp[4]) and same_bits(gen[:3], exp[:3]) and gen[3] == exp[3]
    ref = bn.bootstrap(logw, estimator, mode, k, 0.95, nb, indices=rows)
    assert ref[3] == gen[3]
    np.testing.assert_array_equal(np.isnan(ref[4]), np.isnan(gen[4]))
    scale = 1 + (np.abs(logw).max() if estimator == bn.MEAN else np.abs(np.nan_to_num(ref[4])))
    assert (np.nan_to_num(np.abs(gen[4] - ref[4])) <= 8 * nd * 2.0 ** -53 * scale).all()


def test_repeats_and_addresses_global_resamples(eng):
    logw = sample(1000, seed=3)
    for estimator, mode, k in ((bn.ESS, bn.ONCE, 100.0), (bn.TFEP, bn.RESAMPLE, 1.5), (bn.MEAN, bn.NONE, 1.5)):
        a, b = run(eng, logw, estimator, mode, k, 16, seed=11), run(eng, logw, estimator, mode, k, 16, seed=11)
        assert same_bits(a[4], b[4]) and same_bits(a[:3], b[:3]) and a[3] == b[3]
        assert not np.isnan(a[4]).any() and len(set(a[4])) > 8
        assert same_bits(run(eng, logw, estimator, mode, k, 257, seed=11)[4][:3], run(eng, logw, estimator, mode, k, 3, seed=11)[4])
        assert same_bits(run(eng, logw, estimator, mode, k, 4, first=5, seed=11)[4], a[4][5:9])
        assert not same_bits(run(eng, logw, estimator, mode, k, 16, seed=12)[4], a[4])
        # the point estimate and its kept count do not depend on the resamples
        p0 = run(eng, logw, estimator, mode, k, 0)
        assert same_bits(p0[0], a[0]) and p0[3] == a[3] and np.isnan(p0[1]) and np.isnan(p0[2]) and p0[4] is None


def test_memory_modes_agree_and_wrappers_take_cuda_tensors(eng):
    import torch
    ti = pkg()
    obs = ti.observables
    logw = sample(4097, seed=5)
    dev = torch.from_numpy(logw).cuda()
    rows = bn.draw_rows(1, 0, 6, 300, 4097)
    for estimator, mode, k, idx in ((bn.ESS, bn.ONCE, 1.5, None), (bn.TFEP, bn.RESAMPLE, 100.0, None), (bn.MEAN, bn.RESAMPLE, 1.5, rows)):
        h = run(eng, logw, estimator, mode, k, 6, seed=4, indices=idx)
        d = run(eng, dev, estimator, mode, k, 6, seed=4, indices=None if idx is None else torch.from_numpy(idx).cuda())
        assert d[4].is_cuda and d[4].dtype == torch.float64
        assert same_bits(h[4], d[4].cpu().numpy()) and same_bits(h[:3], d[:3]) and h[3] == d[3]
    # the wrappers: phi formed in fp64, -phi rounded to fp32 once, then the same call
    rs = np.random.RandomState(8)
    E0, E1, dl = rs.standard_normal(500) * 2 + 100, rs.standard_normal(500) * 2 + 101, rs.standard_normal(500).astype(np.float32)
    neg_phi = (-(E1 - E0 + dl.astype(np.float64))).astype(np.float32)
    t = lambda a: torch.from_numpy(a).cuda()
    for fn, est, mode in ((obs.ess_ti, bn.ESS, bn.ONCE), (obs.free_energy_tfep, bn.TFEP, bn.RESAMPLE)):
        want = run(eng, neg_phi, est, mode, 100.0, 32, seed=9)
        for args in ((E0, E1, dl), (t(E0), t(E1), t(dl))):
            r = fn(*args, k=100.0, n_boot=32, seed=9)
            got = r.estimates.cpu().numpy() if hasattr(r.estimates, "is_cuda") else r.estimates
            assert same_bits(got, want[4]) and same_bits([r.point, *r.ci], want[:3]) and r.n_kept == want[3]
        assert same_bits(fn(E0, E1, dl, n_boot=4, seed=9).estimates, run(eng, neg_phi, est, bn.NONE, 1.5, 4, seed=9)[4])      # k=None: no filter
    r = obs.free_energy_bg(t(E0), t(dl), t(E1), t(dl), k=100.0, n_boot=32, seed=3)
    a = run(eng, (-(E0 + dl.astype(np.float64))).astype(np.float32), bn.MEAN, bn.RESAMPLE, 100.0, 32, seed=6)
    b = run(eng, (-(E1 + dl.astype(np.float64))).astype(np.float32), bn.MEAN, bn.RESAMPLE, 100.0, 32, seed=7)
    assert same_bits(r.estimates.cpu().numpy(), b[4] - a[4]) and r.point == b[0] - a[0] and r.n_kept == (a[3], b[3])
    np.testing.assert_allclose(r.ci, np.percentile(b[4] - a[4], [2.5, 97.5]), rtol=1e-12)
    assert abs(r.point - 1.0) < 0.5 and r.ci[0] < r.point < r.ci[1]


def test_generator_statistics(eng):
    """n = 4096, logw ~ N(0, 0.5^2), MEAN, no filter, 2000 resamples: the standard deviation of the estimates lies within 10 % of
    s / sqrt(n) -- six standard errors of a standard deviation estimated from 2000 draws (1 / sqrt(2 * 2000) = 1.6 % each)."""
    logw = sample(4096, seed=21, sd=0.5)
    point, lo, hi, kept, est = run(eng, logw, bn.MEAN, bn.NONE, 1.5, 2000, seed=2)
    s = logw.astype(np.float64).std()
    sd = est.std(ddof=1)
    print(f"sd of the estimates {sd:.6f}, s / sqrt(n) {s / 64:.6f}, ratio {sd / (s / 64):.4f}")
    assert kept == 4096 and abs(point + logw.astype(np.float64).mean()) < 1e-12
    assert abs(sd / (s / 64) - 1) < 0.10
    assert lo < point < hi and abs((hi - lo) / (2 * 1.96 * s / 64) - 1) < 0.15
    assert abs(est.mean() - point) < 6 * (s / 64) / np.sqrt(2000)


def test_device_side_refusals_leave_the_handle_usable(eng):
    ti = pkg()
    logw = sample(300, seed=9)
    good = run(eng, logw, bn.ESS, bn.ONCE, 1.5, 4, seed=1)
    rows = bn.draw_rows(1, 0, 4, 50, 300)
    for bad_value, mode in ((300, bn.NONE), (-1, bn.RESAMPLE), (2 ** 31 - 1, bn.NONE), (good[3], bn.ONCE)):      # ONCE: the population is the survivors
        bad = rows.copy()
        bad[2, 49] = bad_value
        out = np.full(4, 7.0)
        with pytest.raises(ti._lib.TiError, match="idx entry outside") as e:
            eng.bootstrap(logw, bn.ESS, mode, 1.5, 0.95, 4, 0, 0, bad, out_boot=out)
        assert e.value.code == ti._lib.TI_E_ARG and (out == 7.0).all()
    nan = logw.copy()
    nan[123] = np.inf
    with pytest.raises(ti._lib.TiError, match="non-finite logw at index 123") as e:
        run(eng, nan, bn.TFEP, bn.RESAMPLE, 1.5, 4)
    assert e.value.code == ti._lib.TI_E_NAN
    again = run(eng, logw, bn.ESS, bn.ONCE, 1.5, 4, seed=1)
    assert same_bits(again[4], good[4]) and same_bits(again[:3], good[:3]) and again[3] == good[3]
    assert again[3] < 300                                                     # the filter did drop samples here
