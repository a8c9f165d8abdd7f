"""GPU: Hutchinson's divergence estimator (include/ti_hip.h ti_painn_drift_div_est, ti_painn_rollout_dlogp_est).

The probes are regenerated on the host with oracle.normal (the same Philox normal as the EM noise, probe index in the step slot,
component 3a + c), and the estimate is checked against (1/k) sum_p eps_p^T (J eps_p) formed from fp64 oracle JVPs along the same
probes.  The bar is the exact path's (2e-5), normalised by S = (1/k) sum |eps_i (J eps)_i| instead of |div|: the off-diagonal
terms cancel in the sum, so its round-off scales with the sum of absolute terms.
"""
import numpy as np
import pytest

from conftest import golden_weights, load_golden, pkg, rel_l2
from oracle import oracle

pytestmark = pytest.mark.gpu

EST_ATOL = 2e-5
SEED = 20261015


def probes(seed, traj0, B, k, A):
    """eps [B, k, A, 3] of the header's definition, from the host Philox normal"""
    eps = np.empty((B, k, A * 3), np.float32)
    for b in range(B):
        for p in range(k):
            for i in range(3 * A):
                eps[b, p, i] = 1.0 if oracle.normal(seed, traj0 + b, p, i) >= 0.0 else -1.0
    return eps.reshape(B, k, A, 3)


def make_pair(g, precision="f32"):
    ti = pkg()
    args = (int(g["variant"]), int(g["F"]), int(g["L"]), int(g["A"]), g["edge_src"], g["edge_dst"], g["edge_type"], g["atom_ids"], golden_weights(g))
    kw = dict(temp_length=float(g["temp_length"]), temperatures=g["temperatures"])
    return ti.engine.PainnEngine(*args, precision=precision, **kw), oracle.PainnOracle(*args, **kw)


def batch_of(g, B, seed=3):
    """B distinct molecules around the fixture's first one (small displacements), with its conditioning"""
    x = np.repeat(g["x"][:1], B, axis=0) + 0.05 * np.random.RandomState(seed).standard_normal((B,) + g["x"].shape[1:])
    cond = None if g["cond"] is None or g["cond"].ndim == 0 else np.repeat(g["cond"][:1], B, axis=0)
    return x.astype(np.float32), cond


def oracle_estimate(orc, x, t, cond, eps):
    """(est [B], S [B]) with fp64 oracle JVPs along every probe"""
    k = eps.shape[1]
    terms = np.stack([eps[:, p].astype(np.float64) * orc.jvp(x, eps[:, p], t, cond, precision=64)[1] for p in range(k)], axis=1)
    return terms.sum(axis=(2, 3)).mean(axis=1), np.abs(terms).sum(axis=(2, 3)).mean(axis=1)


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("name", ["div_ambient_full", "div_latent_multi", "div_ambient_f256", "div_range_big_f128", "div_lnaff_harsh_f128"])
def test_estimator_identity_vs_fp64_oracle(name, precision):
    g = load_golden(name)
    eng, orc = make_pair(g, precision)
    A, t, B, off = int(g["A"]), float(g["t"]), 3, 1000
    x, cond = batch_of(g, B)
    b_exact, _ = eng.drift_div(x, t, cond)
    for k in (1, 3, 8):
        eps = probes(SEED, off, B, k, A)
        b, est = eng.drift_div_est(x, t, cond, n_probes=k, probe_seed=SEED, traj_offset=off)
        np.testing.assert_array_equal(b, b_exact)                     # the primal pipeline is the exact path's
        ref, S = oracle_estimate(orc, x, t, cond, eps)
        assert (np.abs(est - ref) < EST_ATOL * (S + 1.0)).all(), (k, est, ref, S)
        # per-molecule times: a uniform vector is the scalar-t call bit for bit
        _, est_tv = eng.drift_div_est(x, np.full(B, t, np.float32), cond, n_probes=k, probe_seed=SEED, traj_offset=off)
        np.testing.assert_array_equal(est_tv, est)
    # a different traj_offset draws different probes, and the estimate follows them
    _, est0 = eng.drift_div_est(x, t, cond, n_probes=1, probe_seed=SEED, traj_offset=0)
    ref0, S0 = oracle_estimate(orc, x, t, cond, probes(SEED, 0, B, 1, A))
    assert (np.abs(est0 - ref0) < EST_ATOL * (S0 + 1.0)).all()


def test_unbiased_with_the_closed_form_variance():
    """One molecule under M = 8192 trajectory ids, k = 1: the mean of the estimates lies within 5 standard errors of the library's
    exact divergence, and their variance within 20 % of 2 sum_{i != j} ((J_ij + J_ji) / 2)^2 from the fp64 oracle's full Jacobian."""
    g = load_golden("div_ambient_full")
    eng, orc = make_pair(g, "f32")
    A, t, M = int(g["A"]), float(g["t"]), 8192
    x1, c1 = g["x"][:1], g["cond"][:1]
    _, div = eng.drift_div(x1, t, c1)
    _, est = eng.drift_div_est(np.repeat(x1, M, axis=0), t, np.repeat(c1, M, axis=0), n_probes=1, probe_seed=SEED, traj_offset=0)
    est = est.astype(np.float64)
    n = 3 * A
    J = np.empty((n, n))
    for j in range(n):
        e = np.zeros((1, A, 3), np.float32)
        e.reshape(-1)[j] = 1.0
        J[:, j] = orc.jvp(x1, e, t, c1, precision=64)[1].reshape(-1)
    Sym = 0.5 * (J + J.T)
    var = 2.0 * (Sym ** 2).sum() - 2.0 * (np.diag(Sym) ** 2).sum()
    assert abs(np.trace(J) - div[0]) < 2e-5 * (abs(np.trace(J)) + 1.0)
    se = np.sqrt(var / M)
    assert abs(est.mean() - div[0]) < 5.0 * se, (est.mean(), div[0], se)
    assert abs(est.var(ddof=1) / var - 1.0) < 0.2, (est.var(ddof=1), var)


def host_accumulation(eng, path, grid, cond, scheme, div_scale, out_scale, reverse, k, seed):
    """dlogp rows rebuilt on the host from drift_div_est at the returned states (Heun: and at the fp32 predictor state)"""
    s = -1.0 if reverse else 1.0
    dl = np.zeros(path.shape[1])
    rows = [dl.copy()]
    for i in range(len(grid) - 1):
        dt = np.float32(grid[i + 1]) - np.float32(grid[i])
        b1, e1 = eng.drift_div_est(path[i], float(grid[i]), cond, n_probes=k, probe_seed=seed)
        if scheme == "euler":
            dl = dl + float(dt) * (-s * div_scale) * e1.astype(np.float64)
        else:
            xp = path[i] + dt * (np.float32(s) * b1)
            _, e2 = eng.drift_div_est(xp.astype(np.float32), float(grid[i + 1]), cond, n_probes=k, probe_seed=seed)
            dl = dl + 0.5 * float(dt) * (-s * div_scale) * (e1.astype(np.float64) + e2)
        rows.append(dl.copy())
    return np.asarray(rows) * out_scale


@pytest.mark.parametrize("scheme", ["euler", "heun"])
@pytest.mark.parametrize("name", ["div_ambient_small", "div_latent_multi"])
def test_fixed_step_rollouts(name, scheme):
    ti = pkg()
    g = load_golden(name)
    eng, _ = make_pair(g, "f32")
    div_scale = float(g["div_scale"])
    out_scale = 1.0 / div_scale if div_scale != 1.0 else 1.0          # ambient 1e-2 / 1e2, latent 1 / 1
    k = 3
    for reverse in (False, True):
        grid = ti.engine.time_grid(1.0, 0.0, 6) if reverse else ti.engine.time_grid(0.0, 1.0, 6)
        kw = dict(scheme=scheme, div_scale=div_scale, out_scale=out_scale, reverse_ode=reverse)
        path, dl, nfe = eng.rollout_dlogp_est(g["x"], g["cond"], grid, n_probes=k, probe_seed=SEED, **kw)
        path_x, dl_x, nfe_x = eng.rollout_dlogp(g["x"], g["cond"], grid, **kw)
        assert nfe == nfe_x and rel_l2(path - path[0], path_x - path_x[0]) < 1e-6
        ref = host_accumulation(eng, path, grid, g["cond"], scheme, div_scale, out_scale, reverse, k, SEED)
        assert np.abs(dl - ref).max() <= 1e-5 * (np.abs(ref).max() + 1e-6), (reverse, dl, ref)
        assert np.abs(dl[-1]).min() > 0
    # reverse_ode on the same (ascending) grid flips both right-hand sides: one Euler step from the same state
    grid = ti.engine.time_grid(0.0, 0.5, 2)
    kw = dict(scheme="euler", div_scale=div_scale, out_scale=out_scale)
    p_f, d_f, _ = eng.rollout_dlogp_est(g["x"], g["cond"], grid, n_probes=k, probe_seed=SEED, **kw)
    p_r, d_r, _ = eng.rollout_dlogp_est(g["x"], g["cond"], grid, n_probes=k, probe_seed=SEED, reverse_ode=True, **kw)
    np.testing.assert_allclose(p_r[1] - p_r[0], -(p_f[1] - p_f[0]), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(d_r[1], -d_f[1], rtol=1e-6)


@pytest.mark.parametrize("step_control", ["batch", "trajectory"])
def test_dopri5_vs_fine_heun_with_the_same_probes(step_control):
    ti = pkg()
    g = load_golden("div_ambient_small")
    eng, _ = make_pair(g, "f32")
    x, cond = batch_of(g, 5)
    tol, k = 1e-5, 2
    grid = ti.engine.time_grid(0.0, 1.0, 5)
    fine = ti.engine.time_grid(0.0, 1.0, 401)
    eng.set_template(eng.template_for(5))
    path, dl, _ = eng.rollout_dlogp_est(x, cond, grid, n_probes=k, probe_seed=SEED, scheme="dopri5", rtol=tol, atol=tol,
                                        step_control=step_control)
    hp, hdl, _ = eng.rollout_dlogp_est(x, cond, fine, n_probes=k, probe_seed=SEED, scheme="heun")
    assert np.abs(path - hp[::100]).max() < 20 * tol
    # per-trajectory control runs every molecule at the edge of its own tolerance (the shared mode steps at the hardest molecule's
    # pace): its dlogp error against the fine run measured 0.93e-3 here, 1.24x the shared mode's bar -- hence twice that bar
    bar = (20 if step_control == "batch" else 40) * tol * (np.abs(hdl).max() + 1.0)
    assert np.abs(dl - hdl[::100]).max() < bar
    if step_control != "trajectory":
        return
    acc, rej = eng.step_counts(5)
    # every molecule is what it is alone (batch size 1 with its own id) and in any split with matching traj_offset, in any call order
    for b in range(5):
        p1, d1, _ = eng.rollout_dlogp_est(x[b:b + 1], cond[b:b + 1], grid, n_probes=k, probe_seed=SEED, traj_offset=b, scheme="dopri5",
                                          rtol=tol, atol=tol, step_control="trajectory")
        np.testing.assert_array_equal(p1[:, 0], path[:, b])
        np.testing.assert_array_equal(d1[:, 0], dl[:, b])
        a1, r1 = eng.step_counts(1)
        assert (a1[0], r1[0]) == (acc[b], rej[b])
    for lo, hi in ((2, 5), (0, 2)):                                   # the second half first
        ps, ds, _ = eng.rollout_dlogp_est(x[lo:hi], cond[lo:hi], grid, n_probes=k, probe_seed=SEED, traj_offset=lo, scheme="dopri5",
                                          rtol=tol, atol=tol, step_control="trajectory")
        np.testing.assert_array_equal(ps, path[:, lo:hi])
        np.testing.assert_array_equal(ds, dl[:, lo:hi])
    eng.set_template("auto")


@pytest.mark.parametrize("template", ["throughput", "latency"])
def test_hutchinson_race_screen_full_occupancy(template, monkeypatch):
    """4096 molecules x 4 probes fill every CU with two workgroups of each tangent kernel (the regime of
    test_divergence_race_screen_full_occupancy); repeated f32 and f16x2 evaluations must agree per molecule."""
    ti = pkg()
    syn, W = ti.synthetic, ti.weights
    monkeypatch.setenv("TI_TEMPLATE", template)
    F, L, A, B, k = 128, 2, 18, 4096, 4
    src, dst, et = syn.fully_connected_template(A)
    flat = W.flatten_state_dict(syn.painn_state_dict(0, F, L, 25, seed=F + A), W.painn_param_spec(0, F, L, 25))
    x, cond = syn.molecule_coords(B, A, seed=B), syn.ambient_cond(B, A)
    outs = []
    for prec in ("f32", "f16x2"):
        eng = ti.engine.PainnEngine(0, F, L, A, src, dst, et, np.arange(A), flat, temp_length=100.0, precision=prec)
        outs += [eng.drift_div_est(x, 0.5, cond, n_probes=k, probe_seed=SEED)[1].astype(np.float64) for _ in range(3)]
        eng.close()
    ref = outs[0]
    for o in outs[1:]:
        bad = np.abs(o - ref) > 5e-5 * (np.abs(ref) + 1.0)
        assert not bad.any(), f"{int(bad.sum())} molecules disagree, worst {np.abs(o - ref).max():.2e}"
    np.testing.assert_array_equal(outs[1], outs[0])                   # deterministic within one build
    np.testing.assert_array_equal(outs[4], outs[3])


def test_refusals():
    ti = pkg()
    g = load_golden("div_ambient_small")
    grid = ti.engine.time_grid(0.0, 1.0, 3)
    eng16, _ = make_pair(g, "f16")
    with pytest.raises(ti._lib.TiError) as e:
        eng16.drift_div_est(g["x"], 0.5, g["cond"], n_probes=2)
    assert e.value.code == ti._lib.TI_E_UNSUPPORTED
    with pytest.raises(ti._lib.TiError) as e:
        eng16.rollout_dlogp_est(g["x"], g["cond"], grid, n_probes=2, scheme="heun")
    assert e.value.code == ti._lib.TI_E_UNSUPPORTED
    eng, _ = make_pair(g, "f32")
    for call in (lambda: eng.drift_div_est(g["x"], 0.5, g["cond"], n_probes=0),
                 lambda: eng.drift_div_est(g["x"], np.full(int(g["B"]), 0.5, np.float32), g["cond"], n_probes=0),
                 lambda: eng.rollout_dlogp_est(g["x"], g["cond"], grid, n_probes=0, scheme="heun")):
        with pytest.raises(ti._lib.TiError) as e:
            call()
        assert e.value.code == ti._lib.TI_E_ARG
    with pytest.raises(ti._lib.TiError) as e:
        eng.rollout_dlogp_est(g["x"], g["cond"], grid, n_probes=1, scheme="em")
    assert e.value.code == ti._lib.TI_E_UNSUPPORTED


@pytest.mark.parametrize("name", ["div_ambient_small", "div_latent_multi"])
def test_molecule_integrator_hutchinson(name):
    """MoleculeIntegrator(return_dlogp=True, divergence='hutchinson') with numpy and CUDA-tensor batches: the engine's estimator
    rollout with the batch's trajectory ids."""
    torch = pytest.importorskip("torch")
    from test_gpu_api import golden_batch, state_dict_of
    ti = pkg()
    g = load_golden(name)
    ambient = int(g["variant"]) == 0
    mod = ti.thermo.ambient if ambient else ti.thermo.latent
    kw = dict(n_features=int(g["F"]), score_layers=int(g["L"]), temp_length=int(g["temp_length"]))
    if not ambient:
        kw["temperatures"] = [int(x) for x in g["temperatures"]]
    b = mod.cPaiNN(**kw)
    b.load_state_dict(state_dict_of(g))
    batch = golden_batch(g, "atoms" if ambient else "atom_number")
    integ = mod.MoleculeIntegrator(b=b, method="heun", n_step=5, return_dlogp=True, divergence="hutchinson", n_probes=2, probe_seed=SEED)
    res = integ.rollout(batch, traj_offset=7)
    dl = res[1].numpy()
    eng, _ = make_pair(g, "f32")
    scale = float(g["div_scale"])
    _, ref, _ = eng.rollout_dlogp_est(g["x"], g["cond"], ti.engine.time_grid(0.0, 1.0, 5), n_probes=2, probe_seed=SEED, traj_offset=7,
                                      scheme="heun", div_scale=scale, out_scale=1e2 if ambient else 1.0)
    assert np.allclose(dl, ref, rtol=1e-5, atol=1e-6 * (np.abs(ref).max() + 1.0))
    exact = mod.MoleculeIntegrator(b=b, method="heun", n_step=5, return_dlogp=True).rollout(batch)[1].numpy()
    assert not np.array_equal(dl, exact)
    cuda = type(batch)(**{kk: (v.cuda() if torch.is_tensor(v) else v) for kk, v in vars(batch).items()})
    res_c = integ.rollout(cuda, traj_offset=7)
    assert res_c[1].is_cuda
    np.testing.assert_allclose(res_c[1].cpu().numpy(), dl, rtol=1e-6, atol=1e-6 * (np.abs(dl).max() + 1.0))


def test_drivers_write_dlogps_with_the_estimator(tmp_path):
    import os
    import types
    ti = pkg()
    g = load_golden("ambient_small")
    A, F, L = int(g["A"]), int(g["F"]), int(g["L"])
    traj = np.random.RandomState(1).standard_normal((8, 7, A, 3)) * 0.3
    os.makedirs(tmp_path / "test")
    np.save(tmp_path / "test" / "00031.npy", traj)
    ds = ti.data.MDQM9SamplerDataset("00031.npy", str(tmp_path), "test", T0=1000, T1=300, scale=False, cutoff=1000)
    b = ti.thermo.ambient.cPaiNN(n_features=F, score_layers=L, temp_length=100)
    b.load_state_dict(ti.synthetic.painn_state_dict(0, F, L, 25, int(g["seed"])))
    cfg = types.SimpleNamespace(seed=0, batch_size=4, n_steps=3, atol=1e-5, rtol=1e-5, return_dlogp=1, method="heun",
                                data_save_path=str(tmp_path / "out"), data_save_name="h", divergence="hutchinson", n_probes=2, probe_seed=5)
    samples, _ = ti.drivers.sample_ambient(cfg, b, ds)
    dl = np.load(tmp_path / "out" / "dlogps_h.npy")
    assert samples.shape == (7, 3, A, 3) and dl.shape == (7,) and np.isfinite(dl).all() and np.abs(dl).max() > 0
