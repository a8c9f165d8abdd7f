"""ti_obs_bg_logw on the GPU: bit for bit against the numpy restatement (tests/bg_numpy.py) over the lane and workgroup edges, every
NULL combination of the optional arguments, the independence of a row from its batch, memory space, handle and call, the reference's
own numbers (tests/golden/bg_reference.npz) through observables.log_prior / bg_logw / ess_bg, MoleculeIntegrator.log_prob, and the
drivers' observables["bg"] key end to end.

Measured on an MI355X: every bit comparison holds; against the reference's functions the worst errors are 0.008 and 0.960 of the two
bounds of tests/test_bg_host.py; log_prob lies 8.9e-5 from the right sign's value and 0.62 from the wrong one's.
ess_bg, whose point estimate comes from the fp64 log-weights, reaches 0.06 of the reference bound."""
import ctypes as C
import os
import types

import numpy as np
import pytest

from conftest import load_golden, pkg
import bg_numpy as bgn
from test_bg_host import check_against_fixture, fixture_cases

pytestmark = pytest.mark.gpu

MS = (1, 3, 63, 64, 65, 96, 128, 129, 200)          # lanes with 0, 1, 2 and a ragged third term
BS = (1, 3, 4, 5, 1027)                             # fewer waves than a workgroup, one workgroup, one more, a ragged last workgroup
EPS = 2.0 ** -53


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same(a, b):
    """bit equality, any NaN matching any NaN (the payload of a NaN that an addition produced is the hardware's)"""
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(a)[~nan], bits(b)[~nan])


@pytest.fixture(scope="module")
def eng():
    return pkg().observables._service_engine(0)


@pytest.fixture(scope="module")
def mol_eng():
    ti = pkg()
    syn, W = ti.synthetic, ti.weights
    A = 3
    src, dst, et = syn.fully_connected_template(A)
    flat = W.flatten_state_dict(syn.painn_state_dict(0, 32, 1, 25, seed=1), W.painn_param_spec(0, 32, 1, 25))
    return ti.engine.PainnEngine(0, 32, 1, A, src, dst, et, np.arange(A), flat, temp_length=100.0)


def batch_rows(B, m, seed=0):
    """(z [B, m], u1, nd_bg, nd_ti, index of the inf row or None, of the NaN row or None): normal rows with, as far as B allows, a
    zero row, a row of fp32 denormals, a row of +-3e38, and -- with neighbours on both sides -- one inf row and one NaN row"""
    rs = np.random.RandomState(1000 * m + B + seed)
    z = rs.standard_normal((B, m)).astype(np.float32)
    u1 = 5.0 * rs.standard_normal(B)
    nb, nt = (3.0 * rs.standard_normal(B)).astype(np.float32), (3.0 * rs.standard_normal(B)).astype(np.float32)
    inf_row = nan_row = None
    if B >= 3:
        inf_row = B // 2
        z[inf_row, m // 2] = np.inf
    if B >= 5:
        z[0] = 0.0
        z[B - 1] = (np.arange(m) % 7 + 1).astype(np.float32) * np.float32(1.4e-45)            # denormals: their squares are exact in fp64
    if B >= 1027:
        z[1] = np.where(np.arange(m) % 2, 3e38, -3e38).astype(np.float32)
        nan_row = B - 2                                                                      # in the ragged last workgroup
        z[nan_row, 0] = np.nan
        u1[7], nb[8], nt[9] = np.inf, -np.inf, np.nan                                        # non-finite terms pass through to their rows
    return z, u1, nb, nt, inf_row, nan_row


# ---- 1. bits against the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", MS)
def test_bits_against_the_restatement(eng, m):
    torch = pytest.importorskip("torch")
    for B in BS:
        z, u1, nb, nt, inf_row, nan_row = batch_rows(B, m)
        ref_lp, ref_lw = bgn.bg_logw(z, u1, nb, nt)
        lw, lp = eng.bg_logw(z, u1, nb, nt, logpz=True)
        assert lp.dtype == np.float64 and lw.dtype == np.float32 and lp.shape == lw.shape == (B,)
        assert same(lp, ref_lp) and same(lw, ref_lw), (m, B)
        dev = lambda a: torch.from_numpy(a).cuda()
        lw_d, lp_d = eng.bg_logw(dev(z), dev(u1), dev(nb), dev(nt), logpz=True)
        assert lw_d.is_cuda and lp_d.is_cuda and lp_d.dtype == torch.float64 and lw_d.dtype == torch.float32
        assert same(lp_d.cpu().numpy(), ref_lp) and same(lw_d.cpu().numpy(), ref_lw), (m, B)
        if inf_row is not None:
            assert lp[inf_row] == -np.inf and np.isfinite(lp[[inf_row - 1, inf_row + 1]]).all()
        if nan_row is not None:
            assert np.isnan(lp[nan_row]) and np.isnan(lw[nan_row]) and np.isfinite(lp[[nan_row - 1, nan_row + 1]]).all()
            assert np.isfinite(lp[[7, 8, 9]]).all() and lw[7] == -np.inf and lw[8] == np.inf and np.isnan(lw[9])
            clean, _, _, _, _, _ = batch_rows(B, m)
            clean[inf_row], clean[nan_row] = 1.0, 1.0                                        # the neighbours keep their bits
            lp_clean = eng.bg_logw(clean, logpz=True)[1]
            near = [inf_row - 1, inf_row + 1, nan_row - 1, nan_row + 1]
            assert same(lp_clean[near], lp[near])


def test_shapes_are_flattened_per_row(eng):
    z = np.random.RandomState(3).standard_normal((5, 6, 3)).astype(np.float32)
    assert same(eng.bg_logw(z, logpz=True)[1], bgn.log_prior(z.reshape(5, 18)))
    assert same(eng.bg_logw(z[:, 0, 0], logpz=True)[1], bgn.log_prior(z[:, 0, :1]))          # [B]: m = 1
    assert same(pkg().observables.log_prior(z), bgn.log_prior(z.reshape(5, 18)))


# ---- 2. optional arguments ---------------------------------------------------------------------------------------------------------
def test_every_null_combination(eng):
    ti = pkg()
    L = ti._lib.lib()
    B, m = 6, 65
    z, u1, nb, nt, _, _ = batch_rows(B, m, seed=5)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    for mask in range(8):
        a1, a2, a3 = (u1 if mask & 1 else None), (nb if mask & 2 else None), (nt if mask & 4 else None)
        ref_lp, ref_lw = bgn.bg_logw(z, a1, a2, a3)
        for want_lp, want_lw in ((True, True), (True, False), (False, True)):
            lp, lw = np.full(B, 7.0), np.full(B, 7.0, np.float32)
            rc = L.ti_obs_bg_logw(eng.h, p(z), B, m, p(a1), p(a2), p(a3), p(lp) if want_lp else None, p(lw) if want_lw else None, ti._lib.MEM_HOST)
            assert rc == ti._lib.TI_OK, ti._lib.last_error()
            assert same(lp, ref_lp) if want_lp else (lp == 7.0).all(), mask
            assert same(lw, ref_lw) if want_lw else (lw == 7.0).all(), mask
        assert same(eng.bg_logw(z, a1, a2, a3), ref_lw)
    # the refusals behind a live handle leave the outputs alone
    lp, lw = np.full(B, 7.0), np.full(B, 7.0, np.float32)
    for args in ((None, B, m, p(lp), p(lw), 0), (p(z), B, m, None, None, 0), (p(z), 0, m, p(lp), p(lw), 0), (p(z), B, 0, p(lp), p(lw), 0),
                 (p(z), B, 65537, p(lp), p(lw), 0), (p(z), B, m, p(lp), p(lw), 7)):
        assert L.ti_obs_bg_logw(eng.h, args[0], args[1], args[2], None, None, None, args[3], args[4], args[5]) == ti._lib.TI_E_ARG
    assert (lp == 7.0).all() and (lw == 7.0).all()


def test_mixed_memory_is_refused(eng):
    torch = pytest.importorskip("torch")
    z, u1, nb, nt, _, _ = batch_rows(4, 9)
    with pytest.raises(ValueError, match="same memory space"):
        eng.bg_logw(torch.from_numpy(z).cuda(), torch.from_numpy(u1).cuda(), nb)
    with pytest.raises(ValueError, match="same memory space"):
        eng.bg_logw(z, u1, torch.from_numpy(nb).cuda())
    with pytest.raises(TypeError, match="u1"):
        eng.bg_logw(torch.from_numpy(z).cuda(), u1)


# ---- 3. row independence -----------------------------------------------------------------------------------------------------------
def test_a_row_depends_on_its_row_and_m_only(eng, mol_eng):
    torch = pytest.importorskip("torch")
    m = 129
    z, u1, nb, nt, _, _ = batch_rows(37, m, seed=9)
    z = np.where(np.isfinite(z), z, np.float32(1.5))
    lw, lp = eng.bg_logw(z, u1, nb, nt, logpz=True)
    perm = np.random.RandomState(2).permutation(37)
    lw_p, lp_p = eng.bg_logw(z[perm], u1[perm], nb[perm], nt[perm], logpz=True)                # another place in the batch
    assert same(lp_p, lp[perm]) and same(lw_p, lw[perm])
    for rows in ([5], [36, 0, 17], list(range(9, 14))):                                        # another B
        lw_s, lp_s = eng.bg_logw(z[rows], u1[rows], nb[rows], nt[rows], logpz=True)
        assert same(lp_s, lp[rows]) and same(lw_s, lw[rows])
    big = np.concatenate([z] * 120)                                                            # 4440 rows, 1110 workgroups of one trip each
    assert same(eng.bg_logw(big, logpz=True)[1], np.tile(lp0 := eng.bg_logw(z, logpz=True)[1], 120)) and same(lp0, lp)
    small = np.ascontiguousarray(z[:, :3])                                                     # 70 300 rows: workgroups take a second trip
    assert same(eng.bg_logw(np.concatenate([small] * 1900), logpz=True)[1], np.tile(eng.bg_logw(small, logpz=True)[1], 1900))
    dev = lambda a: torch.from_numpy(a).cuda()
    lw_d, lp_d = eng.bg_logw(dev(z), dev(u1), dev(nb), dev(nt), logpz=True)                    # device memory
    assert same(lp_d.cpu().numpy(), lp) and same(lw_d.cpu().numpy(), lw)
    lw_m, lp_m = mol_eng.bg_logw(z, u1, nb, nt, logpz=True)                                    # a molecule handle, m not 3A
    assert same(lp_m, lp) and same(lw_m, lw)
    lw_2, lp_2 = eng.bg_logw(z, u1, nb, nt, logpz=True)                                        # a second call
    assert same(lp_2, lp) and same(lw_2, lw)


# ---- 4. the reference's numbers ----------------------------------------------------------------------------------------------------
def test_fixture_log_prior_and_logw():
    obs = pkg().observables
    worst = [0.0, 0.0]
    for c in fixture_cases():
        z = c["z"].reshape(-1, c["A"], 3)
        lp = obs.log_prior(z)
        lw = obs.bg_logw(z, c["E1"], c["nd_bg"], None if c["name"].endswith("noti") else c["nd_ti"])
        assert lp.dtype == np.float64 and lw.dtype == np.float32
        check_against_fixture(c, lp, lw, worst)
        ref_lp, ref_lw = bgn.bg_logw(c["z"], c["E1"], c["nd_bg"], c["nd_ti"])
        assert same(lp, ref_lp) and same(lw, ref_lw)
    print(f"GPU against the reference: worst errors {worst[0]:.3f} and {worst[1]:.3f} of the bounds")


def _ess_of(logw, keep=None):
    w = np.exp(logw.astype(np.float64) - logw.astype(np.float64).max())
    w = w if keep is None else w[keep]
    return np.square(w.sum()) / np.square(w).sum()


def test_bg_ess_is_the_ess_of_the_unrounded_log_weights(eng):
    """ti_obs_bg_ess against calc_ESS restated in numpy on the same fp64 log-weights, within 8 n 2^-53 (1 + ess) (two sums of n
    terms and the device's exp against the host's); the keep mask; host against device memory and a repeat bit for bit; the refusals."""
    torch = pytest.importorskip("torch")
    ti = pkg()
    for B in (1, 5, 255, 256, 257, 1000):                                                    # around the workgroup's 256 threads
        z, u1, nb, nt, _, _ = batch_rows(B, 27, seed=3)
        z = np.where(np.isfinite(z), z, np.float32(0.5))
        lp = eng.bg_logw(z, logpz=True)[1]
        keep = (np.arange(B) % 3 != 1).astype(np.uint8) if B > 1 else None
        for a1, a2, a3, kp in ((u1, nb, nt, None), (u1, nb, None, keep), (None, None, None, keep)):
            zero = np.zeros(B)
            l = -((((zero if a1 is None else a1) + lp) + (zero if a2 is None else a2.astype(np.float64))) + (zero if a3 is None else a3.astype(np.float64)))
            sel = np.ones(B, bool) if kp is None else kp != 0
            w = np.exp(l[sel] - l[sel].max())
            want = np.square(w.sum()) / np.square(w).sum()
            got, kept = eng.bg_ess(lp, a1, a2, a3, kp)
            assert kept == sel.sum() and abs(got - want) <= 8 * sel.sum() * EPS * (1 + want), (B, got, want)
            dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
            assert eng.bg_ess(dev(lp), dev(a1), dev(a2), dev(a3), dev(kp)) == (got, kept) == eng.bg_ess(lp, a1, a2, a3, kp)
    bad = u1.copy()
    bad[[700, 12]] = np.nan, np.inf
    with pytest.raises(ti._lib.TiError, match="index 12"):
        eng.bg_ess(lp, bad, nb, nt)
    skip = np.ones(B, np.uint8)
    skip[[700, 12]] = 0                                                                      # a non-finite entry the mask drops is not read
    assert eng.bg_ess(lp, bad, nb, nt, skip)[1] == B - 2
    with pytest.raises(ti._lib.TiError, match="no molecule"):
        eng.bg_ess(lp, u1, nb, nt, np.zeros(B, np.uint8))
    L, E = ti._lib.lib(), ti._lib.TI_E_ARG
    out = C.c_double(7.0)
    assert L.ti_obs_bg_ess(eng.h, None, B, None, None, None, None, C.byref(out), None, 0) == E
    assert L.ti_obs_bg_ess(eng.h, C.c_void_p(lp.ctypes.data), 0, None, None, None, None, C.byref(out), None, 0) == E
    assert L.ti_obs_bg_ess(eng.h, C.c_void_p(lp.ctypes.data), B, None, None, None, None, C.byref(out), None, 3) == E
    assert L.ti_obs_bg_ess(None, C.c_void_p(lp.ctypes.data), B, None, None, None, None, C.byref(out), None, 0) == E and out.value == 7.0


def test_fixture_ess_bg_against_the_reference():
    """ess_bg against calc_ESS of the reference's fp64 weights, for k = None and for k = 1.5 where the fixture's guard holds, within
    the bound tests/test_gpu_boot.py uses for the ess point estimate: 8 n 2^-53 (1 + |ess|), n the kept count.

    The point estimate is taken from the unrounded fp64 log-weights (ti_obs_bg_ess).  Taken from the fp32 log-weights, as the
    bootstrap's own point is, it misses this bound by factors 1.4e3 .. 3.2e7: the one rounding moves an ESS by up to 2e-6 relative.
    Worst error on the numpy restatement of the fp64 path: 0.015 of the bound for k = None, 0.062 for k = 1.5."""
    obs = pkg().observables
    ratios = []
    for c in fixture_cases():
        z = c["z"].reshape(-1, c["A"], 3)
        r = obs.ess_bg(z, c["E1"], c["nd_bg"], c["nd_ti"], n_boot=8)
        assert r.n_kept == c["w"].size and 1.0 <= r.ci[0] <= r.ci[1] <= c["w"].size
        ratios.append((c["name"], "none", abs(r.point - c["ess"]) / (8 * c["w"].size * EPS * (1 + abs(c["ess"])))))
        if c["ess_k_ok"]:
            rk = obs.ess_bg(z, c["E1"], c["nd_bg"], c["nd_ti"], k=c["k"], n_boot=0)
            assert rk.n_kept == c["kept_k"]
            ratios.append((c["name"], "k", abs(rk.point - c["ess_k"]) / (8 * c["kept_k"] * EPS * (1 + abs(c["ess_k"])))))
    for name, mode, ratio in ratios:
        print(f"ess_bg against the reference, {name} ({mode}): error {ratio:.3g} of the bound")
    assert all(ratio <= 1.0 for _, _, ratio in ratios), ratios
    # the interval and the resamples are the bootstrap's on the fp32 log-weights
    c = fixture_cases()[1]
    z = c["z"].reshape(-1, c["A"], 3)
    a, b = obs.ess_bg(z, c["E1"], c["nd_bg"], c["nd_ti"], k=c["k"], n_boot=8), obs.bootstrap(obs.bg_logw(z, c["E1"], c["nd_bg"], c["nd_ti"]), "ess", k=c["k"], n_boot=8)
    assert a.ci == b.ci and a.n_kept == b.n_kept and same(a.estimates, b.estimates) and abs(a.point - b.point) <= 1e-5 * b.point


def test_free_energy_bg_tfep_is_the_named_fold():
    obs = pkg().observables
    rs = np.random.RandomState(4)
    E0, E1 = 5.0 * rs.standard_normal(200), 5.0 * rs.standard_normal(200)
    n0, n1 = (3.0 * rs.standard_normal(200)).astype(np.float32), (3.0 * rs.standard_normal(200)).astype(np.float32)
    phi = E1 + n1.astype(np.float64) - E0 - n0.astype(np.float64)                              # calc_phis_bg_tfep
    want = -np.log(np.mean(np.exp(-phi)))                                                      # calc_tfep_dF with unit weights
    got = obs.free_energy_bg_tfep(E0, n0, E1, n1, n_boot=8)
    assert abs(got.point - want) <= 1e-5 * (1 + abs(want)) and got.n_kept == 200
    same_as = obs.free_energy_tfep(E0, E1, n1.astype(np.float64) - n0.astype(np.float64), n_boot=8)
    assert abs(got.point - same_as.point) <= 1e-5 * (1 + abs(want))


# ---- 5. log_prob -------------------------------------------------------------------------------------------------------------------
def latent_model(g):
    ti = pkg()
    from test_gpu_api import state_dict_of
    b = ti.thermo.latent.cPaiNN(n_features=int(g["F"]), score_layers=int(g["L"]), temp_length=int(g["temp_length"]),
                                temperatures=[int(x) for x in g["temperatures"]])
    b.load_state_dict(state_dict_of(g))
    return b


def test_log_prob_composition_and_sign():
    """div_latent_multi (F = 32, L = 2, A = 6), heun on 9 grid points, 4 molecules of centred N(0, 1) noise (RandomState(11)): forward
    from z0 to (x1, nd), then log_prob(x1).  On the CPU oracle the composed density lies 8.6e-5 from log_prior(z0) + nd and at
    least 0.62 from log_prior(z0) - nd (a factor 7 330 where the condition asks for 10)."""
    ti = pkg()
    obs = ti.observables
    g = load_golden("div_latent_multi")
    b = latent_model(g)
    B, A, n_step = 4, int(g["A"]), 9
    z0 = np.random.RandomState(11).standard_normal((B, A, 3)).astype(np.float32)
    template = (g["edge_src"], g["edge_dst"], g["edge_type"])
    T = int(g["cond"][0, 0, 0])
    kw = dict(b=b, method="heun", n_step=n_step, atol=1e-5, rtol=1e-5)
    fwd = ti.thermo.latent.MoleculeIntegrator(return_dlogp=True, **kw)
    batch = ti.data.make_batch("latent", z0, template, T=T, atom_ids=g["atom_ids"])
    xts, dlogp, _ = fwd.rollout(batch)
    x1, nd = np.asarray(xts[-1]).reshape(B, A, 3), np.asarray(dlogp[-1]).astype(np.float64)
    back = ti.data.make_batch("latent", x1, template, T=T, atom_ids=g["atom_ids"])
    plain = ti.thermo.latent.MoleculeIntegrator(return_dlogp=False, **kw)                      # log_prob brings its own settings
    lp = plain.log_prob(back)
    assert isinstance(lp, np.ndarray) and lp.dtype == np.float64 and lp.shape == (B,)
    assert (plain.return_dlogp, plain.reverse_ode, plain.start, plain.end) == (False, False, 0.0, 1.0)
    # the hand composition: the same field on the descending grid, then the prior of where it ends
    inv = ti.thermo.latent.MoleculeIntegrator(return_dlogp=True, start=1.0, end=0.0, **kw)
    zts, d, _ = inv.rollout(back)
    hand = obs.log_prior(np.ascontiguousarray(np.asarray(zts[-1]).reshape(B, 3 * A))) - np.asarray(d[-1]).astype(np.float64)
    assert same(lp, hand)
    prior0 = obs.log_prior(np.ascontiguousarray(batch.x0.reshape(B, 3 * A)))
    right, wrong = np.abs(lp - (prior0 + nd)), np.abs(lp - (prior0 - nd))
    print(f"log_prob: |lp - (prior + nd)| <= {right.max():.2e}, |lp - (prior - nd)| >= {wrong.min():.2e}")
    assert (10 * right < wrong).all(), (right, wrong)


# ---- 6. the drivers ----------------------------------------------------------------------------------------------------------------
def soft_forcefield(A, to_nm):
    """tests/ff_numpy.py's synthetic species with every energy scale multiplied by one factor (the energy is linear in them), chosen so
    that the reduced energies of N(0, 1) clouds at 300 K spread by 2: the weights of a handful of molecules then stay comparable and
    no bootstrap resample loses all of its weight"""
    import ff_numpy as fn
    ff = {k: np.array(v, copy=True) for k, v in fn.synthetic_forcefield(A).items()}
    clouds = np.random.RandomState(5).standard_normal((64, A, 3)).astype(np.float32)
    lam = 2.0 / fn.energies(clouds, to_nm, ff, T=np.full(64, 300.0, np.float32))[0].std()
    ff["bond_par"][:, 1] *= lam; ff["angle_par"][:, 1] *= lam; ff["torsion_par"][:, 2] *= lam
    ff["particles"][:, 0] *= np.sqrt(lam); ff["particles"][:, 2] *= lam
    ff["exceptions"][:, 2] *= lam; ff["exceptions"][:, 4] *= lam
    return ff


def test_drivers_with_the_bg_key(tmp_path):
    """sample_latent with the key, then sample_ambient chained on its files with energy + bg: 6 molecules of the fixture's A = 9,
    4 grid points.  Every written logw_bg is bg_logw of the run's own files, bit for bit; without the key the file sets are today's."""
    ti = pkg()
    obs = ti.observables
    from test_gpu_forcefield import write_xml
    import ff_numpy as fn
    A, n, to_nm = 9, 6, 3.0
    scale = 1.0 / to_nm
    ff = soft_forcefield(A, to_nm)
    x = np.random.RandomState(6).standard_normal((1, A, 3)).astype(np.float32)                 # fixes A and the graph only
    write_xml(ff, tmp_path / "ff.xml")
    key = {"forcefield": str(tmp_path / "ff.xml"), "scale": scale}
    g = load_golden("div_latent_multi")
    b = latent_model(g)
    ds = ti.data.LatentSamplerDataset(x[0], T=300, n_samples=n, seed=3)
    common = dict(seed=0, batch_size=3, n_steps=4, atol=1e-5, rtol=1e-5, return_dlogp=1, method="euler")
    lat = tmp_path / "latent"
    name = "mol_00031_300k"                                                                   # what load_latent_trajectory reads
    # without the key: today's files
    ti.drivers.sample_latent(types.SimpleNamespace(**common, data_save_path=str(tmp_path / "plain"), data_save_name=name), b, ds)
    assert sorted(os.listdir(tmp_path / "plain")) == [f"dlogps_{name}_forward.npy", f"samples_{name}_forward.npy"]
    cfg = types.SimpleNamespace(**common, data_save_path=str(lat), data_save_name=name, observables={"bg": key, "bootstrap": 16})
    samples = ti.drivers.sample_latent(cfg, b, ds)
    assert sorted(os.listdir(lat)) == [f"E1s_samples_{name}_forward.npy", f"bg_{name}_forward.npz", f"dlogps_{name}_forward.npy",
                                       f"samples_{name}_forward.npy"]
    np.testing.assert_array_equal(bits(samples), bits(np.load(tmp_path / "plain" / f"samples_{name}_forward.npy")))
    E1, dl = np.load(lat / f"E1s_samples_{name}_forward.npy"), np.load(lat / f"dlogps_{name}_forward.npy")
    assert samples.shape == (n, 4, A, 3) and E1.shape == dl.shape == (n,) and E1.dtype == np.float64 and np.isfinite(E1).all()
    z0 = np.ascontiguousarray(samples[:, 0])
    with np.load(lat / f"bg_{name}_forward.npz") as f:
        assert sorted(f.files) == ["E1", "ess_bg", "ess_bg_ci", "log_pz", "logw_bg"]
        assert f["log_pz"].shape == f["logw_bg"].shape == (n,) and f["log_pz"].dtype == np.float64 and f["logw_bg"].dtype == np.float32
        assert same(f["E1"], E1) and same(f["log_pz"], obs.log_prior(z0)) and same(f["logw_bg"], obs.bg_logw(z0, E1, dl))
        assert same(f["logw_bg"], bgn.bg_logw(z0.reshape(n, -1), E1, dl)[1])
        want = _ess_of(f["logw_bg"])
        assert abs(float(f["ess_bg"]) - want) <= 1e-5 * want and 1.0 <= f["ess_bg_ci"][0] <= f["ess_bg_ci"][1] <= n
    # the written energies are those of the written end states at T = 300 K
    ref, _, S, _ = fn.energies(samples[:, -1], to_nm, ff, T=np.full(n, 300.0, np.float32))
    assert (np.abs(E1 - ref) <= 1e-11 * S.sum(axis=1) / (fn.R_GAS * 300.0)).all()

    # the chain: the ambient map on the latent run's files
    amb = ti.thermo.ambient.cPaiNN(n_features=32, score_layers=1, temp_length=100)
    amb.load_state_dict(ti.synthetic.painn_state_dict(0, 32, 1, 25, 4))
    chained = ti.data.MDQM9SamplerDataset("00031.npy", "", "test", T0=300, T1=400, scale=True, cutoff=1000, use_latent_trajs=True,
                                          latent_traj_path=str(lat))
    assert chained.use_latent_trajs and len(chained) == n            # scale=True: the end states are taken as they are
    cv = {"descriptors": [["dist", 0, 1]], "bins": 4, "bootstrap": 16}
    ti.drivers.sample_ambient(types.SimpleNamespace(**common, data_save_path=str(tmp_path / "amb_plain"), data_save_name="p", observables=cv), amb, chained)
    assert sorted(os.listdir(tmp_path / "amb_plain")) == ["dlogps_p.npy", "latent_dlogps_p.npy", "latent_noises_p.npy", "observables_p.npz", "samples_p.npy"]
    with np.load(tmp_path / "amb_plain" / "observables_p.npz") as f:
        assert sorted(f.files) == ["cv", "edges", "ess", "ess_boot", "ess_ci", "hist"]
    out = tmp_path / "amb"
    ti.drivers.sample_ambient(types.SimpleNamespace(**common, data_save_path=str(out), data_save_name="c",
                                                    observables={**cv, "energy": key, "bg": True}), amb, chained)
    assert sorted(os.listdir(out)) == ["E0s_samples_c.npy", "E1s_samples_c.npy", "dlogps_c.npy", "latent_dlogps_c.npy", "latent_noises_c.npy",
                                       "observables_c.npz", "samples_c.npy"]
    E1a, dla = np.load(out / "E1s_samples_c.npy"), np.load(out / "dlogps_c.npy")
    zl, dll = np.load(out / "latent_noises_c.npy"), np.load(out / "latent_dlogps_c.npy")
    assert zl.shape == (n, A, 3) and dll.shape == dla.shape == (n,) and np.abs(zl).max() > 0 and np.abs(dll).max() > 0
    with np.load(out / "observables_c.npz") as f:
        assert sorted(f.files) == sorted(["cv", "edges", "ess", "ess_boot", "ess_ci", "hist", "E0", "E1", "logw", "ess_ti", "ess_ti_ci",
                                          "log_pz", "logw_bg", "ess_bg", "ess_bg_ci"])
        assert same(f["log_pz"], obs.log_prior(zl)) and same(f["logw_bg"], obs.bg_logw(zl, E1a, dll, dla))
        assert same(f["logw_bg"], bgn.bg_logw(zl.reshape(n, -1), E1a, dll, dla)[1])
        want = _ess_of(f["logw_bg"])
        assert abs(float(f["ess_bg"]) - want) <= 1e-5 * want and 1.0 <= f["ess_bg_ci"][0] <= f["ess_bg_ci"][1] <= n
    # a dataset without the latent trajectories is refused before the rollout
    os.makedirs(tmp_path / "test")
    np.save(tmp_path / "test" / "00031.npy", np.broadcast_to(x[0].astype(np.float64), (8, n, A, 3)).copy())
    md = ti.data.MDQM9SamplerDataset("00031.npy", str(tmp_path), "test", T0=300, T1=400, scale=False, cutoff=1000)
    with pytest.raises(ValueError, match="use_latent_trajs"):
        ti.drivers.sample_ambient(types.SimpleNamespace(**common, data_save_path=str(tmp_path / "no"), data_save_name="n",
                                                        observables={**cv, "energy": key, "bg": True}), amb, md)
    assert not os.path.exists(tmp_path / "no")
