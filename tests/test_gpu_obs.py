"""GPU: the observables layer (include/ti_hip.h ti_obs_*) against its fp64 restatement tests/obs_numpy.py -- collective variables
(uniform and mixed-species batches), importance weights, the deterministic weighted histogram, the per-row observer of every
rollout entry point and of the integrator mirrors, and the weighted-RMSD-histogram check of tests/test_gpu_observables.py restated
through the product API.

Bounds.  Device and oracle compute in fp64 from the same fp32 inputs, so a CV differs by the fp32 rounding of the output (6e-8
relative) plus, for an RMSD near 0, sqrt(1e-16 e0 / A) ~ 3e-8 of the coordinate scale (the eigenvalue's absolute error under the
square root): |dev - ref| <= 1e-6 (1 + |ref|) for distances, angles and torsions (modulo 2 pi), <= 1e-6 (1 + sqrt(e0 / A)) for
RMSD, a factor of 10 or more above that.  Histogram bins: fp64 sums of at most B weights <= 1 in another order than numpy's,
1e-12 B absolute; ESS 1e-12 relative."""
import functools
import types

import numpy as np
import pytest

from conftest import pkg, rel_l2
from oracle import oracle
import obs_numpy as on

pytestmark = pytest.mark.gpu

B = 261                                            # one past a 256-thread block
TWO_PI = 2.0 * np.pi


@functools.lru_cache(maxsize=None)
def small_engine(A, F=32, L=1):
    ti = pkg()
    syn, W = ti.synthetic, ti.weights
    flat = W.flatten_state_dict(syn.painn_state_dict(0, F, L, 25, seed=1), W.painn_param_spec(0, F, L, 25))
    return ti.engine.PainnEngine(0, F, L, A, *syn.fully_connected_template(A), np.arange(A), flat, temp_length=100.0)


def rotation(rs):
    q, _ = np.linalg.qr(rs.standard_normal((3, 3)))
    return q * np.sign(np.linalg.det(q))


def descriptors(A):
    """K = 6 mixing all four kinds; indices wrap for the small molecules (a repeated atom gives a degenerate but defined value or NaN
    on both sides alike)."""
    a = lambda i: i % A
    return [("rmsd",), ("dist", a(0), a(1)), ("angle", a(0), a(1), a(2)), ("torsion", a(0), a(1), a(2), a(3)), ("dist", a(A - 1), a(0)),
            ("torsion", a(3), a(2), a(1), a(0))]


def problem(A, shape="random"):
    """x [B,A,3] fp32 and ref [A,3]: molecule 0 a pure rotation + translation of ref, molecule 1 its mirror image, the rest noise
    around rotated copies."""
    rs = np.random.RandomState(100 + A)
    ref = rs.standard_normal((A, 3)) * 1.3
    if shape == "collinear":
        ref = np.outer(np.arange(A) - 0.7, [0.6, -0.3, 0.9])
    elif shape == "planar":
        ref[:, 2] = 0.0
    x = np.stack([ref @ rotation(rs).T for _ in range(B)]) + rs.standard_normal((B, 1, 3)) + 0.2 * rs.standard_normal((B, A, 3))
    x[0] = ref @ rotation(rs).T + [4.0, -2.5, 1.0]
    x[1] = ref * [1.0, 1.0, -1.0]
    return x.astype(np.float32), ref.astype(np.float32)


def well_defined(x, desc):
    """[B,K] bool, decided on the oracle side: False where the value is 0/0 or a quotient of round-off -- an angle with an arm of
    length 0, a torsion with a collinear triple (the reference itself divides by zero there), as the wrapped indices of the one-, two-
    and three-atom molecules and the exactly collinear copies produce.  Such entries have no value to compare; everything else is."""
    x = np.asarray(x, np.float64)
    ok = np.ones((x.shape[0], len(desc)), bool)
    unit = lambda v: np.linalg.norm(v, axis=-1)
    for k, (kind, i, j, kk, l) in enumerate(np.asarray(desc).tolist()):
        if kind == on.ANGLE:
            ok[:, k] = (unit(x[:, i] - x[:, j]) > 1e-6) & (unit(x[:, kk] - x[:, j]) > 1e-6)
        elif kind == on.TORSION:
            b1, b2, b3 = x[:, j] - x[:, i], x[:, kk] - x[:, j], x[:, l] - x[:, kk]
            ok[:, k] = (unit(np.cross(b1, b2)) > 1e-3 * unit(b1) * unit(b2)) & (unit(np.cross(b2, b3)) > 1e-3 * unit(b2) * unit(b3)) \
                & (unit(b1) > 0) & (unit(b2) > 0) & (unit(b3) > 0)
    return ok


def check_cv(dev, ref_cv, desc, scale, tag, defined=None):
    """the derived bounds; prints the worst figure of every column before asserting"""
    assert dev.dtype == np.float32 and dev.shape == ref_cv.shape
    for k, d in enumerate(desc):
        kind, r, g = d[0], ref_cv[:, k], dev[:, k].astype(np.float64)
        use = np.ones(r.shape, bool) if defined is None else defined[:, k]
        nan = np.isnan(r) | ~use
        assert (np.isnan(g) == np.isnan(r))[use].all(), (tag, k, d)
        diff = np.abs(g - r)[~nan]
        if kind == on.TORSION:
            diff = np.minimum(diff, TWO_PI - diff)
        bar = 1e-6 * (1.0 + (scale if kind == on.RMSD else np.abs(r))[~nan])
        worst = float((diff / bar).max()) if diff.size else 0.0
        print(f"cv {tag} column {k} kind {kind}: worst |dev - ref| / bound = {worst:.3e}")
        assert worst <= 1.0, (tag, k, d, worst)


@pytest.mark.parametrize("A,shape", [(1, "random"), (2, "random"), (3, "collinear"), (3, "planar"), (9, "random"), (25, "random")])
def test_cvs_match_the_fp64_restatement(A, shape):
    ti = pkg()
    eng = small_engine(A)
    x, ref = problem(A, shape)
    desc = ti.observables.encode_descriptors(descriptors(A))
    cv = eng.collective_variables(x, desc, ref=ref)
    want = on.collective_variables(x, desc, ref)
    defined = well_defined(x, desc)
    assert defined[:, [0, 1, 4]].all() and (A < 9 or defined[2:].all())
    check_cv(cv, want, desc, on.rmsd_scale(x, ref), f"A={A} {shape}", defined)
    # sqrt cancellation: a rotated and translated copy is at RMSD 0 to 1e-6 of the coordinate scale (fp32 sums give 1e-3)
    scale0 = on.rmsd_scale(x[:1], ref)[0]
    print(f"A={A} {shape}: rmsd of the rotated copy {cv[0, 0]:.3e}, scale {scale0:.3e}; mirror image {cv[1, 0]:.6e} vs {want[1, 0]:.6e}")
    assert cv[0, 0] < 1e-6 * max(scale0, 1e-30) or (A == 1 and cv[0, 0] == 0.0)
    if A >= 9:                                               # a chiral frame: the mirror image is not at 0
        assert want[1, 0] > 0.1 and abs(cv[1, 0] - want[1, 0]) <= 1e-6 * (1 + scale0)
    # bit-identical re-run; row b unchanged when the batch is permuted
    np.testing.assert_array_equal(eng.collective_variables(x, desc, ref=ref).view(np.uint32), cv.view(np.uint32))
    perm = np.random.RandomState(3).permutation(B)
    np.testing.assert_array_equal(eng.collective_variables(x[perm], desc, ref=ref).view(np.uint32), cv[perm].view(np.uint32))


def test_rmsd_selection_device_tensors_and_refusals():
    torch = pytest.importorskip("torch")
    ti = pkg()
    A = 9
    eng = small_engine(A)
    x, ref = problem(A)
    sel = np.array([1, 1, 0, 1, 0, 1, 1, 1, 0], np.int32)
    x[5] = x[0]
    x[5, sel == 0] += 7.0                                   # dropped atoms do not count
    desc = ti.observables.encode_descriptors([("rmsd",), ("dist", 2, 4)])
    xd = torch.from_numpy(x).cuda()
    cv = eng.collective_variables(xd, desc, ref=ref, select=sel)
    assert cv.is_cuda and tuple(cv.shape) == (B, 2)
    want = on.collective_variables(x, desc, ref, sel)
    check_cv(cv.cpu().numpy(), want, desc, on.rmsd_scale(x, ref, sel), "select")
    assert max(cv[5, 0].item(), want[5, 0]) < 1e-6 * on.rmsd_scale(x[5:6], ref, sel)[0]
    np.testing.assert_array_equal(eng.collective_variables(x, desc, ref=ref, select=sel).view(np.uint32), cv.cpu().numpy().view(np.uint32))
    E = ti._lib.TiError
    for bad, msg in (([("dist", 0, A)], "atom index"), ([("coord", 0)], "adw"), ([("rmsd",)], "needs ref")):
        with pytest.raises(E, match=msg) as ei:
            eng.collective_variables(x, bad)
        assert ei.value.code == ti._lib.TI_E_ARG
    import ctypes as C
    L = ti._lib.lib()
    raw = np.array([[7, 0, 0, 0, 0]], np.int32)             # an unknown kind, handed to the library as it is
    out = np.zeros((B, 1), np.float32)
    rc = L.ti_obs_cv(eng.h, ti._lib.iptr(raw), 1, None, None, C.c_void_p(x.ctypes.data), B, C.c_void_p(out.ctypes.data), 0)
    assert rc == ti._lib.TI_E_ARG and "unknown kind" in ti._lib.last_error()
    adw = ti.observables._service_engine(0)
    for bad, msg in (([("torsion", 0, 0, 0, 0)], "COORD"), ([("rmsd",)], "COORD"), ([("coord", 1)], "component")):
        with pytest.raises(E, match=msg) as ei:
            adw.collective_variables(np.zeros(4, np.float32), bad)
        assert ei.value.code == ti._lib.TI_E_ARG
    xs = np.linspace(-1, 1, 7).astype(np.float32)
    np.testing.assert_array_equal(adw.collective_variables(xs, [("coord", 0)])[:, 0], xs)
    with pytest.raises(ValueError):
        adw.weighted_histogram(xs, None, 8, (1.0, 1.0))
    h, t = np.zeros(8), np.zeros(3)
    dp = C.POINTER(C.c_double)
    for n_bins, lo, hi in ((0, 0.0, 1.0), (257, 0.0, 1.0), (8, 1.0, 1.0), (8, 2.0, 1.0)):
        rc = L.ti_obs_hist(adw.h, C.c_void_p(xs.ctypes.data), 1, None, 7, n_bins, lo, hi, h.ctypes.data_as(dp), t.ctypes.data_as(dp), 0)
        assert rc == ti._lib.TI_E_ARG, (n_bins, lo, hi)


def test_ragged_batch_real_values_pads_and_nan():
    """set_molecules batch of the test_gpu_species_edges kinds (1, 2, 21, 22, 25 atoms at A = 25)."""
    import test_gpu_species_edges as E
    ti = pkg()
    A = E.A
    ms = [E.mix(B, junk) for junk in E.JUNK]
    eng = E.engine(ms[0])
    ref = np.random.RandomState(5).standard_normal((A, 3)).astype(np.float32)
    sel = (np.arange(A) % 3 != 1).astype(np.int32)
    sel[0] = 1
    desc = ti.observables.encode_descriptors([("rmsd",), ("dist", 0, 1), ("angle", 0, 1, 20), ("torsion", 0, 1, 20, 21), ("dist", 24, 0),
                                              ("torsion", 21, 2, 1, 0)])
    cvs = [eng.collective_variables(m.x, desc, ref=ref, select=sel) for m in ms]
    for cv in cvs[1:]:                                       # three pad contents: the same bits (NaN patterns included)
        np.testing.assert_array_equal(cv.view(np.uint32), cvs[0].view(np.uint32))
    m = ms[0]
    want = on.collective_variables(m.x, desc, ref, sel, n_atoms=m.n_atoms)
    # each molecule alone: the oracle on its real atoms only, no pads anywhere
    for b in range(2 * E.NK):
        n = int(m.n_atoms[b])
        alone = on.collective_variables(m.x[b:b + 1, :n], desc[:1], ref[:n], sel[:n])
        assert alone[0, 0] == want[b, 0]
    scale = np.array([on.rmsd_scale(m.x[b:b + 1, :n], ref[:n], sel[:n])[0] for b, n in enumerate(m.n_atoms)])
    check_cv(cvs[0], want, desc, scale, "ragged")
    nan = np.isnan(cvs[0])
    assert not nan[:, 0].any()                               # RMSD runs over the real selected atoms
    np.testing.assert_array_equal(nan[:, 1], m.n_atoms < 2)
    np.testing.assert_array_equal(nan[:, 2], m.n_atoms < 21)
    np.testing.assert_array_equal(nan[:, 3], m.n_atoms < 22)
    np.testing.assert_array_equal(nan[:, 4], m.n_atoms < 25)
    assert (cvs[0][m.n_atoms == 1, 0] == 0).all()            # one atom: both sets are their own centroid


# ------------------------------------------------------------------------------------------------------------ weights, histogram
def hist_problem(Bn, bins, lo, hi):
    """values with some placed exactly on interior edges, on lo and on hi, below, above, NaN and inf; logw spanning 60 nats.  The range
    is chosen so that the edges are fp32 numbers; every other value keeps 1e-6 clear of every edge (asserted on the oracle side)."""
    rs = np.random.RandomState(Bn + bins)
    v = rs.uniform(lo - 0.2 * (hi - lo), hi + 0.2 * (hi - lo), Bn)
    e = on.bin_edges(bins, lo, hi)
    assert (e.astype(np.float32).astype(np.float64) == e).all()
    near = on.edge_clearance(v.astype(np.float32), bins, lo, hi) < 2e-6
    v[near] += 4e-6
    v = v.astype(np.float32)
    placed = np.zeros(Bn, bool)
    spots = list(e[1:-1][:: max(1, (bins - 1) // 5)]) + [lo, hi, hi, lo - 1.0, hi + 3.0, np.nan, np.inf, -np.inf]
    for i, s in enumerate(spots):
        v[7 * i + 3] = s
        placed[7 * i + 3] = True
    free = np.isfinite(v) & ~placed
    assert (on.edge_clearance(v[free], bins, lo, hi) > 1e-6).all()          # bin assignment is unambiguous for every entry
    logw = (rs.uniform(-30.0, 30.0, Bn)).astype(np.float32)
    logw[0], logw[1] = -30.0, 30.0
    return v, logw


@pytest.mark.parametrize("Bn", [261, 3500])
@pytest.mark.parametrize("bins,lo,hi", [(1, -1.0, 3.0), (12, -1.5, 4.5), (80, -2.5, 2.5), (256, 0.0, 4.0)])
def test_weighted_histogram_and_ess(Bn, bins, lo, hi):
    ti = pkg()
    eng = ti.observables._service_engine(0)
    v, logw = hist_problem(Bn, bins, lo, hi)
    w, ess = eng.importance_weights(logw)
    w_ref, ess_ref = on.importance_weights(logw)
    assert np.isfinite(w).all() and np.isfinite(ess)
    print(f"B={Bn}: ess {ess:.12e} vs {ess_ref:.12e}; max |w - w_ref| {np.abs(w - w_ref).max():.3e}")
    assert abs(ess - ess_ref) <= 1e-12 * ess_ref
    assert np.abs(w - w_ref).max() <= 1e-6 * w_ref.max()              # fp32 output
    for lw in (logw, None):
        hist, tails = eng.weighted_histogram(v, lw, bins, (lo, hi))
        h_ref, t_ref = on.weighted_histogram(v, lw, bins, lo, hi)
        print(f"B={Bn} bins={bins} weighted={lw is not None}: max |hist - ref| {np.abs(hist - h_ref).max():.3e}, tails {tails}")
        assert np.abs(hist - h_ref).max() <= 1e-12 * Bn and np.abs(tails - t_ref).max() <= 1e-12 * Bn
        assert abs(hist.sum() - (1.0 - tails.sum())) <= 1e-12 * Bn
        assert (tails > 0).all()
        h2, t2 = eng.weighted_histogram(v, lw, bins, (lo, hi))
        np.testing.assert_array_equal(hist.view(np.uint64), h2.view(np.uint64))
        np.testing.assert_array_equal(tails.view(np.uint64), t2.view(np.uint64))
    if bins == 12:                                           # a strided column on the device gives the same bits as the host copy
        torch = pytest.importorskip("torch")
        cv = torch.zeros((Bn, 3), device="cuda")
        cv[:, 1] = torch.from_numpy(v).cuda()
        hd, td = eng.weighted_histogram(cv[:, 1], torch.from_numpy(logw).cuda(), bins, (lo, hi))
        hw, tw = eng.weighted_histogram(v, logw, bins, (lo, hi))
        np.testing.assert_array_equal(hd.view(np.uint64), hw.view(np.uint64))
        np.testing.assert_array_equal(td.view(np.uint64), tw.view(np.uint64))
        f = ti.observables.free_energy_profile(v, logw, bins, (lo, hi))
        np.testing.assert_allclose(f, on.free_energy_profile(v, logw, bins, lo, hi), rtol=0, atol=1e-9)


def test_a_strided_column_gives_the_same_bits_from_host_and_device_memory():
    """ti_obs_hist on column 1 of a [70, 3] array, 8 bins: a host call packs the column before the upload, a device call reads it in
    place through the stride.  Both give the bits of the contiguous column, with weights (the shift and the sums run first) and
    without (the scratch is sized by the call itself).  The neighbouring columns lie outside the range, so a wrong stride or a
    wrong column would move weight into the tails; the bound against the restatement is the module's, 1e-12 B."""
    import torch
    eng = pkg().observables._service_engine(0)
    Bn, bins, lo, hi = 70, 8, -1.0, 3.0
    rs = np.random.RandomState(70)
    v = rs.uniform(lo - 0.8, hi + 0.8, Bn)
    v[on.edge_clearance(v.astype(np.float32), bins, lo, hi) < 2e-6] += 4e-6
    v = v.astype(np.float32)
    assert (on.edge_clearance(v, bins, lo, hi) > 1e-6).all()
    logw = rs.uniform(-30.0, 30.0, Bn).astype(np.float32)
    cv = np.empty((Bn, 3), np.float32)
    cv[:, 0], cv[:, 1], cv[:, 2] = lo - 5.0, v, hi + 5.0
    cvd = torch.from_numpy(cv).cuda()
    assert cv[:, 1].strides == (12,) and cvd[:, 1].stride(0) == 3
    for lw in (logw, None):
        h_ref, t_ref = on.weighted_histogram(v, lw, bins, lo, hi)
        hh, th = eng.weighted_histogram(cv[:, 1], lw, bins, (lo, hi))
        hd, td = eng.weighted_histogram(cvd[:, 1], None if lw is None else torch.from_numpy(lw).cuda(), bins, (lo, hi))
        hc, tc = eng.weighted_histogram(v, lw, bins, (lo, hi))
        print(f"weighted={lw is not None}: max |hist - ref| {np.abs(hh - h_ref).max():.3e}, tails {th}")
        assert np.abs(hh - h_ref).max() <= 1e-12 * Bn and np.abs(th - t_ref).max() <= 1e-12 * Bn
        assert th[0] > 0 and th[1] > 0 and hh.min() > 0
        for h2, t2 in ((hd, td), (hc, tc)):
            np.testing.assert_array_equal(hh.view(np.uint64), h2.view(np.uint64))
            np.testing.assert_array_equal(th.view(np.uint64), t2.view(np.uint64))


def test_non_finite_logw_is_refused_with_its_index():
    ti = pkg()
    eng = ti.observables._service_engine(0)
    logw = np.linspace(-3, 3, B).astype(np.float32)
    logw[200] = np.nan
    logw[230] = np.inf
    for call in (lambda: eng.importance_weights(logw), lambda: eng.weighted_histogram(np.zeros(B, np.float32), logw, 8, (-1, 1))):
        with pytest.raises(ti._lib.TiError, match="index 200") as ei:
            call()
        assert ei.value.code == ti._lib.TI_E_NAN


# ------------------------------------------------------------------------------------------------------------ observer
@functools.lru_cache(maxsize=None)
def obs_model():
    """the test_gpu_observables model: F = 32, L = 2, A = 9, B = 96"""
    ti = pkg()
    syn, W = ti.synthetic, ti.weights
    F, L, A, Bm = 32, 2, 9, 96
    src, dst, et = syn.fully_connected_template(A)
    flat = W.flatten_state_dict(syn.painn_state_dict(0, F, L, 25, seed=3), W.painn_param_spec(0, F, L, 25))
    eng = ti.engine.PainnEngine(0, F, L, A, src, dst, et, np.arange(A), flat, temp_length=100.0)
    x0, cond = syn.molecule_coords(Bm, A, seed=5), syn.ambient_cond(Bm, A)
    return types.SimpleNamespace(eng=eng, x0=x0, cond=cond, A=A, B=Bm, args=(0, F, L, A, src, dst, et, np.arange(A), flat))


OBS_DESC = [("rmsd",), ("dist", 0, 8), ("angle", 1, 2, 3), ("torsion", 0, 1, 2, 3)]
N_GRID, EVERY = 8, 2                                         # 7 steps: observer rows at grid points 0, 2, 4, 6, 7


@pytest.mark.parametrize("case", ["euler", "heun", "em", "rk4", "dopri5", "dlogp", "hutchinson"])
def test_observer_rows_are_the_cvs_of_the_saved_rows(case):
    ti = pkg()
    m = obs_model()
    eng, ref = m.eng, m.x0[0]
    grid = ti.engine.time_grid(0.0, 1.0, N_GRID)
    if case == "dlogp":
        run = lambda: eng.rollout_dlogp(m.x0, m.cond, grid, scheme="heun", save_every=1, div_scale=1e-2, out_scale=1e2)
    elif case == "hutchinson":
        run = lambda: eng.rollout_dlogp_est(m.x0, m.cond, grid, n_probes=2, probe_seed=9, scheme="euler", save_every=1, div_scale=1e-2, out_scale=1e2)
    else:
        kw = dict(eps=0.02, seed=4) if case == "em" else dict(rtol=1e-4, atol=1e-4) if case == "dopri5" else {}
        run = lambda: eng.rollout(m.x0, m.cond, grid, scheme=case, save_every=1, **kw)
    plain = run()
    rows = int(ti._lib.lib().ti_rollout_rows(N_GRID, EVERY))
    assert rows == 5
    cv = np.full((rows, m.B, len(OBS_DESC)), np.nan, np.float32)
    eng.set_observer(OBS_DESC, ref=ref, every=EVERY, out=cv)
    try:
        seen = run()
    finally:
        eng.set_observer(None)
    for a, b in zip(plain, seen):                            # path, (dlogp,) n_fevals: bit-identical with and without the observer
        if isinstance(a, np.ndarray):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
        else:
            assert a == b
    path = seen[0]
    for r, i in enumerate([0, 2, 4, 6, 7]):
        want = eng.collective_variables(path[i], OBS_DESC, ref=ref)
        np.testing.assert_array_equal(cv[r].view(np.uint32), want.view(np.uint32), err_msg=f"{case} row {r}")
    again = run()                                            # detached: nothing is written any more
    np.testing.assert_array_equal(again[0].view(np.uint32), plain[0].view(np.uint32))


def test_observer_adw_coord_and_save_every_independence():
    ti = pkg()
    from conftest import load_golden
    ga = load_golden("adw_ctor_h64")
    spec = ti.weights.adw_param_spec(int(ga["hidden"]), int(ga["num_layers"]))
    flat = ti.weights.flatten_state_dict({k[4:]: v for k, v in ga.items() if k.startswith("sd::")}, spec, dtype=np.float64)
    eng = ti.engine.AdwEngine(int(ga["hidden"]), int(ga["num_layers"]), flat)
    x0 = np.linspace(-1.8, 1.8, 96).astype(np.float32)
    b0, b1 = np.ones(96, np.float32), np.full(96, 1.25, np.float32)
    grid = ti.engine.time_grid(0.0, 1.0, N_GRID)
    for scheme, dl in (("euler", False), ("dopri5", True)):
        plain = eng.rollout(x0, b0, b1, grid, scheme=scheme, save_every=1, return_dlogp=dl)
        for save_every in (1, 0, 3):
            cv = np.full((5, 96, 1), np.nan, np.float32)
            eng.set_observer([("coord", 0)], every=EVERY, out=cv)
            try:
                seen = eng.rollout(x0, b0, b1, grid, scheme=scheme, save_every=save_every, return_dlogp=dl)
            finally:
                eng.set_observer(None)
            np.testing.assert_array_equal(cv[:, :, 0].view(np.uint32), plain[0][[0, 2, 4, 6, 7]].view(np.uint32), err_msg=f"{scheme} {save_every}")
            assert seen[-1] == plain[-1]
            if save_every == 1:
                for a, b in zip(plain[:-1], seen[:-1]):
                    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_per_trajectory_dopri5_refuses_an_observer_and_works_after_detaching():
    ti = pkg()
    m = obs_model()
    grid = ti.engine.time_grid(0.0, 1.0, 4)
    run = lambda: m.eng.rollout(m.x0, m.cond, grid, scheme="dopri5", step_control="trajectory", rtol=1e-3, atol=1e-3)
    before = run()
    cv = np.zeros((4, m.B, 1), np.float32)
    m.eng.set_observer([("dist", 0, 1)], every=1, out=cv)
    try:
        with pytest.raises(ti._lib.TiError, match="DOPRI5_TRAJ") as ei:
            run()
        assert ei.value.code == ti._lib.TI_E_UNSUPPORTED
    finally:
        m.eng.set_observer(None)
    after = run()
    np.testing.assert_array_equal(before[0].view(np.uint32), after[0].view(np.uint32))


def test_observe_on_the_mirror_classes_cuda_and_mixed_species():
    torch = pytest.importorskip("torch")
    ti = pkg()
    m = obs_model()
    amb = ti.thermo.ambient
    b = amb.cPaiNN(n_features=32, score_layers=2, temp_length=100)
    b.load_state_dict(ti.synthetic.painn_state_dict(0, 32, 2, 25, seed=3))
    tpl = ti.synthetic.fully_connected_template(m.A)
    Bn = 12
    batch = ti.data.make_batch("ambient", m.x0[:Bn], tpl, T0=1000, T1=300)
    dev = types.SimpleNamespace(**{k: (torch.as_tensor(v).cuda() if isinstance(v, np.ndarray) else v) for k, v in vars(batch).items()})
    observe = dict(descriptors=OBS_DESC, ref=m.x0[0], every=EVERY)
    integ = amb.MoleculeIntegrator(b=b, method="heun", n_step=N_GRID, observe=observe)
    xts = integ.rollout(dev)[0]
    assert integ.cv.is_cuda and tuple(integ.cv.shape) == (5, Bn, len(OBS_DESC))
    eng = b.engine_of(ti.thermo._molecule.split_species_batch(batch, "atoms"))
    for r, i in enumerate([0, 2, 4, 6, 7]):
        want = eng.collective_variables(xts[i].reshape(Bn, m.A, 3).contiguous(), OBS_DESC, ref=m.x0[0])
        assert torch.equal(integ.cv[r].view(torch.int32), want.view(torch.int32))
    plain = amb.MoleculeIntegrator(b=b, method="heun", n_step=N_GRID).rollout(dev)[0]
    assert torch.equal(plain.view(torch.int32), xts.view(torch.int32))
    # mixed species: descriptor indices are local to each molecule; molecules lacking a named atom get NaN
    import test_species_host as S
    items, _ = S._species_items()
    mixed = ti.data.concat_species_batches(items)
    sb = ti.thermo._molecule.split_species_batch(mixed, "atoms")
    desc = [("rmsd",), ("dist", 0, 4), ("torsion", 0, 1, 2, 8), ("angle", 9, 10, 11)]
    ref = np.random.RandomState(2).standard_normal((sb.A, 3)).astype(np.float32)
    integ = amb.MoleculeIntegrator(b=b, method="euler", n_step=4, observe=dict(descriptors=desc, ref=ref, every=1))
    xts = integ.rollout(mixed)[0]
    assert integ.cv.shape == (4, sb.B, 4)
    for r in range(4):
        want = on.collective_variables(sb.pad(xts[r], 3), ti.observables.encode_descriptors(desc), ref, n_atoms=sb.n_atoms)
        scale = np.array([on.rmsd_scale(sb.pad(xts[r], 3)[i:i + 1, :n], ref[:n])[0] for i, n in enumerate(sb.n_atoms)])
        check_cv(integ.cv[r], want, ti.observables.encode_descriptors(desc), scale, f"mixed row {r}")
    assert np.isnan(integ.cv[:, sb.n_atoms < 9, 2]).all() and np.isnan(integ.cv[:, sb.n_atoms < 12, 3]).all()
    assert np.isfinite(integ.cv[:, :, :2]).all() and np.isfinite(integ.cv[:, sb.n_atoms == 12]).all()


def test_driver_writes_the_observables_file(tmp_path):
    ti = pkg()
    from conftest import load_golden
    ga = load_golden("adw_ctor_h64")
    net = ti.thermo.adw.FCNetMultiBeta(1, 1, int(ga["hidden"]), int(ga["num_layers"]))
    net.load_state_dict({k[4:]: v for k, v in ga.items() if k.startswith("sd::")})
    n = len(ga["traj_grid"])
    cfg = types.SimpleNamespace(beta0s=[1.0], beta1s=[1.25], solver_type="euler", rtol=1e-4, atol=1e-4, n_step=n, return_dlogp=1,
                                data_save_path=str(tmp_path), model_save_name="v", sampling_epoch=1,
                                observables={"descriptors": [["coord", 0]], "every": 2, "bins": 16})
    xs = ga["x"].astype(np.float32)[:, None]
    initial, samples = ti.drivers.sample_adw(cfg, net, [(xs[:8], np.ones((8, 1))), (xs[8:16], np.ones((8, 1)))])
    out_dir = tmp_path / "v" / "beta_1.0_to_1.25"
    assert sorted(p.name for p in out_dir.iterdir()) == ["dlogps_epoch_1.npy", "initial_samples_epoch_1.npy", "observables_epoch_1.npz",
                                                        "samples_epoch_1.npy"]
    z = np.load(out_dir / "observables_epoch_1.npz")
    rows = int(ti._lib.lib().ti_rollout_rows(n, 2))
    assert z["cv"].shape == (rows, 16, 1) and z["hist"].shape == (1, 16) and z["edges"].shape == (1, 17)
    np.testing.assert_array_equal(z["cv"][-1, :, 0], samples[-1].astype(np.float32))
    np.testing.assert_array_equal(z["cv"][1, :, 0], samples[2].astype(np.float32))
    dl = np.load(out_dir / "dlogps_epoch_1.npy")[-1]
    h_ref, _ = on.weighted_histogram(z["cv"][-1, :, 0], -dl.astype(np.float32), 16, float(z["edges"][0, 0]), float(z["edges"][0, -1]))
    assert np.abs(z["hist"][0] - h_ref).max() < 1e-10 and abs(z["hist"].sum() - 1.0) < 1e-10
    assert abs(float(z["ess"]) - on.importance_weights(-dl.astype(np.float32))[1]) < 1e-9 * 16


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_weighted_rmsd_histogram_through_the_product_api(precision):
    """tests/test_gpu_observables.py::test_weighted_rmsd_histogram_matches_cpu_path with the GPU side computed by the product: rollout,
    CVs, weights and histogram on the device against the oracle rollout run through obs_numpy; the same bars (1e-5 on r, 5e-3 on the
    histogram L1)."""
    ti = pkg()
    m = obs_model()
    eng = ti.engine.PainnEngine(*m.args, temp_length=100.0, precision=precision)
    orc = oracle.PainnOracle(*m.args, temp_length=100.0)
    grid = ti.engine.time_grid(0.0, 1.0, 9)
    path, dl, _ = eng.rollout_dlogp(m.x0, m.cond, grid, scheme="heun", save_every=0, div_scale=1e-2, out_scale=1e2)
    opath, odl, _ = orc.rollout_dlogp(m.x0, m.cond, grid, scheme="heun", save_every=0, div_scale=1e-2)
    assert rel_l2(path[0] - m.x0, opath[0] - m.x0) < 2e-5
    ref = m.x0[0]
    r_c = on.kabsch_rmsd(opath[0], ref)
    lo, hi = 0.0, float(r_c.max() * 1.0001 + 1e-9)
    h_c, t_c = on.weighted_histogram(r_c, -(odl[0].astype(np.float64) * 1e2), 12, lo, hi)
    cv = eng.collective_variables(path[0], [("rmsd",)], ref=ref)
    h_g, t_g = eng.weighted_histogram(cv[:, 0], np.ascontiguousarray(-dl[0]), 12, (lo, hi))
    print(f"{precision}: max |r_gpu - r_cpu| {np.abs(cv[:, 0] - r_c).max():.3e}; histogram L1 {np.abs(h_g - h_c).sum() + np.abs(t_g - t_c).sum():.3e}")
    assert np.abs(cv[:, 0] - r_c).max() < 1e-5
    assert np.abs(h_g - h_c).sum() + np.abs(t_g - t_c).sum() < 5e-3
