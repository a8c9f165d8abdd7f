"""Velocity loss on the GPU (ti_painn_vloss / ti_adw_vloss): every stage against the reference fixtures (tests/golden/vloss_*.npz, made
by make_golden_vloss.py) and the fp64 restatement of tests/vloss_numpy.py, the draws against their definition, determinism and
splitting, the edges, the time profile, that the number ranks a trained checkpoint, and the driver.

Bounds.  S = |(1 - t) x0| + |t x1| + |gamma z| + |mean| (vloss_numpy.interpolate).  Stage one: one fp32 rounding of an fp64 value,
2^-23 S against the restatement (2^-24 S for the rounding, the rest for the fp64 arithmetic, which is far below it), plus the
reference chain's own measured fp32 error xt_ref_err S against the fixture.  Reduce: 2 n_terms 2^-53 sum|terms| (n_terms roundings
of the running sum, as many inside the terms).  Loss against the reference: from the drift bar 1e-5 by Cauchy-Schwarz (below)."""
import os
import types

import numpy as np
import pytest

import vloss_numpy as vn
from conftest import golden_weights, load_golden, pkg, rel_l2

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
PRECISIONS = ["f32", "f16x2"]


# ------------------------------------------------------------------------------------------------ fixtures and engines
def _painn(g, precision="f32"):
    ti = pkg()
    return ti.engine.PainnEngine(int(g["variant"]), int(g["F"]), int(g["L"]), int(g["A"]), g["edge_src"], g["edge_dst"], g["edge_type"],
                                 g["atom_ids"], golden_weights(g), temp_length=float(g["temp_length"]), temperatures=list(g["temperatures"]),
                                 precision=precision)


def _adw(g, precision="f32"):
    ti = pkg()
    H, nl = int(g["hidden"]), int(g["num_layers"])
    flat = ti.weights.flatten_state_dict(ti.synthetic.adw_state_dict(H, nl, int(g["seed"])), ti.weights.adw_param_spec(H, nl), dtype=np.float64)
    return ti.engine.AdwEngine(H, nl, flat, precision=precision)


def _adw_ckpt(name, precision="f32"):
    """(engine, state dict) of an adw fixture that stores its weights (sd::*)"""
    ti = pkg()
    g = load_golden(name)
    sd = {k[4:]: v for k, v in g.items() if k.startswith("sd::")}
    H, nl = int(sd["net.0.weight"].shape[0]), sum(1 for k in sd if k.startswith("net.") and k.endswith(".weight")) - 1
    flat = ti.weights.flatten_state_dict(sd, ti.weights.adw_param_spec(H, nl), dtype=np.float64)
    return ti.engine.AdwEngine(H, nl, flat, precision=precision), sd, H, nl


_ENGINES = {}


def _case_list():
    out = []
    for name in ("vloss_ambient", "vloss_latent_multi", "vloss_adw_h64"):
        for case in load_golden(name)["cases"]:
            out.append((name, str(case)))
    return out


CASES = _case_list()


def _setup(name, case, precision="f32"):
    """-> (engine, call(**kw) -> velocity_loss result, interp(**kw), settings dict, g, c)"""
    g = load_golden(name)
    c = {k.split("::", 1)[1]: v for k, v in g.items() if k.startswith(f"{case}::")}
    key = (name, precision)
    if key not in _ENGINES:
        _ENGINES[key] = _adw(g, precision) if name == "vloss_adw_h64" else _painn(g, precision)
    eng = _ENGINES[key]
    if name == "vloss_ambient":
        s = dict(kind="standard", gamma=case, a=float(g["a"][list(g["cases"]).index(case)]), center="batch")
    elif name == "vloss_latent_multi":
        s = dict(kind="one_sided", gamma="brownian", a=1.0, center="batch")
    else:
        s = dict(kind=case, gamma="brownian", a=float(g["a"]))
    conds = (g["beta0"].astype(np.float32), g["beta1"].astype(np.float32)) if name == "vloss_adw_h64" else (g["cond"],)
    call = lambda **kw: eng.velocity_loss(g["x0"], g["x1"], *conds, **{**s, **kw})
    interp = lambda **kw: eng.interpolate(g["x0"], g["x1"], **{**s, **kw})
    return eng, call, interp, s, g, c


def _vn_kw(s):
    return dict(kind=s["kind"], gamma_kind=s["gamma"], a=s["a"])


def _given(s, c):
    return dict(t=c["t"], z=None if s["kind"] == "one_sided" else c["z"])


def _ref_b(s, c):
    return np.stack([c["bt_plus"], c["bt_minus"]])[: 1 if s["kind"] == "one_sided" else 2]


def _ref_bound(s, g, c):
    """Per-molecule bound of |l_b - l_b^ref| from the drift bar.  l(b) - l(b_ref) = (b - b_ref) . ((b + b_ref) / 2 - v), v = d +- gamma' z,
    so |dl_b| <= (|b+_b| + |d + gamma' z|_b) delta+ + (|b-_b| + |d - gamma' z|_b) delta- with delta+- = 1e-5 |bt_+-| over the batch, plus
    the reduction's own 2 n_terms 2^-53 sum|terms|."""
    B = g["x0"].shape[0]
    f = lambda v: np.asarray(v, np.float64).reshape(B, -1)
    d = f(g["x1"]) - f(g["x0"])
    gz = 0.0 if s["kind"] == "one_sided" else vn.gamma_dot(s["gamma"], s["a"], np.asarray(c["t"], np.float64))[:, None] * f(c["z"])
    nrm = lambda v: np.linalg.norm(v, axis=1)
    bound = (nrm(f(c["bt_plus"])) + nrm(d + gz)) * 1e-5 * np.linalg.norm(c["bt_plus"])
    if s["kind"] == "standard":
        bound = bound + (nrm(f(c["bt_minus"])) + nrm(d - gz)) * 1e-5 * np.linalg.norm(c["bt_minus"])
    _, mag, n_terms = vn.loss(g["x0"], g["x1"], c["t"], c["z"], c["bt_plus"], c["bt_minus"], **_vn_kw(s))
    return bound + 2 * n_terms * U * mag


# ------------------------------------------------------------------------------------------------ 1. interpolate
@pytest.mark.parametrize("name,case", CASES)
def test_interpolate_given_t_z(name, case):
    eng, call, interp, s, g, c = _setup(name, case)
    r = interp(**_given(s, c))
    xt64, S = vn.interpolate(g["x0"], g["x1"], c["t"], c["z"], center=s.get("center", "none"), **_vn_kw(s))
    ref = np.stack([c["xtp"], c["xtm"]])[: xt64.shape[0]].astype(np.float64)
    assert r["xt"].shape == xt64.shape and r["xt"].dtype == np.float32
    assert (np.abs(r["xt"] - ref) <= (float(c["xt_ref_err"]) + 2.0 ** -23) * S).all()
    assert (np.abs(r["xt"] - xt64.astype(np.float32)) <= 2.0 ** -23 * S).all()
    assert np.array_equal(r["t"], c["t"])
    if s["kind"] == "standard":
        assert np.array_equal(r["z"], c["z"])


@pytest.mark.parametrize("center", ["molecule", "none"])
def test_interpolate_other_centrings(center):
    for case in ("brownian", "sig_sum"):
        eng, call, interp, s, g, c = _setup("vloss_ambient", case)
        r = interp(center=center, **_given(s, c))
        xt64, S = vn.interpolate(g["x0"], g["x1"], c["t"], c["z"], center=center, **_vn_kw(s))
        assert (np.abs(r["xt"] - xt64.astype(np.float32)) <= 2.0 ** -23 * S).all()
    eng, call, interp, s, g, c = _setup("vloss_latent_multi", "uniform")
    r = interp(center=center, t=c["t"])
    xt64, S = vn.interpolate(g["x0"], g["x1"], c["t"], center=center, **_vn_kw(s))
    assert (np.abs(r["xt"] - xt64.astype(np.float32)) <= 2.0 ** -23 * S).all()
    if center == "molecule":
        assert np.abs(r["xt"].astype(np.float64).mean(axis=2)).max() < 1e-6


# ------------------------------------------------------------------------------------------------ 2. - 4. drift, reduce, loss
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,case", CASES)
def test_drift_reduce_and_loss_against_the_reference(name, case, precision):
    eng, call, interp, s, g, c = _setup(name, case, precision)
    r = call(returns=("t", "z", "xt", "b"), **_given(s, c))
    ref_b = _ref_b(s, c)
    # 2. the drift on xt: the project's bar for the tv_* fixtures
    assert r["b"].shape == ref_b.shape
    print(f"{name} {case} {precision}: rel_l2(out_b) {rel_l2(r['b'], ref_b):.3e}")
    assert rel_l2(r["b"], ref_b) < 1e-5
    # 3. the reduction is exact: the restatement fed the call's own outputs
    B = g["x0"].shape[0]
    zz = r.get("z")
    bm = r["b"][1] if s["kind"] == "standard" else None
    l, mag, n_terms = vn.loss(g["x0"], g["x1"], r["t"], zz, r["b"][0], bm, **_vn_kw(s))
    assert r["loss"].dtype == np.float64 and r["loss"].shape == (B,)
    assert (np.abs(r["loss"] - l) <= 2 * n_terms * U * mag).all()
    rows = r["rows"]
    assert rows == (B if name == "vloss_adw_h64" else B * int(g["A"]))
    assert abs(r["mean"] - l.sum() / rows) <= 2 * (n_terms + B) * U * mag.sum() / rows
    # 4. against the reference (_ref_bound)
    ref_l = np.asarray(c["row_loss"], np.float64).reshape(B, -1).sum(axis=1)
    bound = _ref_bound(s, g, c)
    print(f"{name} {case} {precision}: max |dl| / bound {np.max(np.abs(r['loss'] - ref_l) / bound):.3e}")
    assert (np.abs(r["loss"] - ref_l) <= bound).all()
    assert abs(r["mean"] - float(c["mean"])) <= bound.sum() / rows


def _mirror_batches(ti, g, x, extra):
    B, A = x.shape[:2]
    kw = dict(x=x.reshape(-1, 3), edge_index=ti.synthetic.batch_edge_index(g["edge_src"], g["edge_dst"], A, B),
              edge_type=np.tile(g["edge_type"].astype(np.int64), B), batch=np.repeat(np.arange(B), A))
    kw.update(extra)
    return types.SimpleNamespace(**kw)


@pytest.mark.parametrize("name,case", CASES)
def test_mirror_forward_against_the_reference_scalar(name, case):
    """thermo.losses forward(...) with t=, z= against the scalar the reference's forward() returned at those draws: within the bound of
    the mean (_ref_bound summed over the rows) plus the reference's own fp32 error, |forward - mean| of the fixture (its fp32 scalar
    against its fp64 rows of the same pieces)."""
    ti = pkg()
    eng, call, interp, s, g, c = _setup(name, case)
    I, Ls = ti.thermo.interpolants, ti.thermo.losses
    if name == "vloss_adw_h64":
        H, nl = int(g["hidden"]), int(g["num_layers"])
        b = ti.thermo.adw.FCNetMultiBeta(1, 1, H, nl)
        b.load_state_dict(ti.synthetic.adw_state_dict(H, nl, int(g["seed"])))
        fn = Ls.StandardVelocityLoss(I.LinearInterpolant(0.9)) if case == "standard" else Ls.OneSidedVelocityLoss(I.OneSidedLinearInterpolant())
        val = fn(b, g["x0"][:, None], g["x1"][:, None], g["beta0"][:, None], g["beta1"][:, None], **_given(s, c))
    else:
        mod = ti.thermo.ambient if name == "vloss_ambient" else ti.thermo.latent
        b = mod.cPaiNN(n_features=int(g["F"]), score_layers=int(g["L"]), temp_length=float(g["temp_length"]), temperatures=list(g["temperatures"]))
        b.load_state_dict(ti.weights.unflatten(golden_weights(g), b._spec))
        B, A = g["x0"].shape[:2]
        ids = np.tile(g["atom_ids"], B)
        if name == "vloss_ambient":
            a_ref = 0.9 if case == "brownian" else s["a"]                     # what the maker passed; the mirror rounds it to float32 as the reference does
            fn = mod.losses.StandardVelocityLoss(mod.interpolants.LinearInterpolant(a_ref, case))
            b0 = _mirror_batches(ti, g, g["x0"], dict(atoms=ids, T=g["cond"][..., 0].reshape(-1)))
            b1 = _mirror_batches(ti, g, g["x1"], dict(atoms=ids, T=g["cond"][..., 1].reshape(-1)))
            val = fn(b0, b1, b, t=np.repeat(c["t"], A), z=c["z"].reshape(-1, 3))
        else:
            fn = mod.losses.OneSidedVelocityLoss(mod.interpolants.OneSidedLinearInterpolant(), t_distr=case)
            bt = _mirror_batches(ti, g, g["x0"], dict(atom_number=ids, T=g["cond"][..., 0].reshape(-1), x0=g["x0"].reshape(-1, 3), x1=g["x1"].reshape(-1, 3)))
            val = fn(bt, b, t=c["t"])
    assert isinstance(val, float) and val == fn.last["mean"]
    r = call(**_given(s, c))
    assert val == r["mean"] and np.array_equal(fn.last["loss"], r["loss"])           # the mirror is the engine call
    assert abs(val - float(c["forward"])) <= _ref_bound(s, g, c).sum() / r["rows"] + abs(float(c["mean"]) - float(c["forward"]))


# ------------------------------------------------------------------------------------------------ 5. draws
def _ulps(a, b):
    return np.abs(a.astype(np.float64) - b) / np.spacing(np.abs(b).astype(np.float32)).astype(np.float64)


def test_drawn_z_equals_oracle_normal_bit_for_bit():
    """out_z against oracle.normal(seed, traj_offset + b, draw, 3a + c) (adw: component 0), bit for bit: the kernel evaluates the
    Box-Muller expression with the host libm's logf / sinf / cosf algorithms restated in fp64 (vloss_kernels.hip vl_normal)."""
    from oracle import oracle
    eng, call, interp, s, g, c = _setup("vloss_ambient", "brownian")
    B, A = g["x0"].shape[:2]
    seed, off, draw = 0x1234567890, 11, 3
    z = interp(seed=seed, traj_offset=off, draw=draw)["z"]
    ref = np.asarray([[[oracle.normal(seed, off + b, draw, 3 * a + k) for k in range(3)] for a in range(A)] for b in range(B)], np.float32)
    ea, _, ia, sa, ga, ca = _setup("vloss_adw_h64", "standard")
    za = ia(seed=seed, traj_offset=off, draw=draw)["z"]
    refa = np.asarray([oracle.normal(seed, off + b, draw, 0) for b in range(ga["x0"].shape[0])], np.float32)
    for tag, got, want in (("molecules", z, ref), ("adw", za, refa)):
        print(f"drawn z, {tag}: {int((got != want).sum())} of {want.size} entries differ from oracle.normal, at most {_ulps(got, want).max():.2f} ulp")
    assert np.array_equal(z, ref)
    assert np.array_equal(za, refa)


def test_drawn_t_follows_its_definition():
    eng, call, interp, s, g, c = _setup("vloss_ambient", "brownian")
    B = g["x0"].shape[0]
    seed, off, draw = 0x1234567890, 11, 3
    assert np.array_equal(interp(seed=seed, traj_offset=off, draw=draw)["t"], vn.draw_t("uniform", seed, off, draw, B))
    for dist in ("beta_half", "beta_2_1"):
        t = interp(seed=seed, traj_offset=off, draw=draw, t_distr=dist)["t"]
        ref = vn.draw_t(dist, seed, off, draw, B)
        assert (np.abs(t - ref) <= np.spacing(ref)).all()
    ea, _, ia, sa, ga, ca = _setup("vloss_adw_h64", "standard")
    assert np.array_equal(ia(seed=seed, traj_offset=off, draw=draw)["t"], vn.draw_t("uniform", seed, off, draw, ga["x0"].shape[0]))


def _small_engine(A=2):
    ti = pkg()
    W, syn = ti.weights, ti.synthetic
    src, dst, ety = syn.fully_connected_template(A)
    flat = W.flatten_state_dict(syn.painn_state_dict(W.AMBIENT, 32, 2, 25, 5), W.painn_param_spec(W.AMBIENT, 32, 2, 25))
    return ti.engine.PainnEngine(W.AMBIENT, 32, 2, A, src, dst, ety, np.arange(A, dtype=np.int32), flat)


def _small():
    if "small" not in _ENGINES:
        _ENGINES["small"] = _small_engine()
    return _ENGINES["small"]


# moments of t: (E t, E t^2, Var t, Var t^2)
MOMENTS = {"uniform": (1 / 2, 1 / 3, 1 / 12, 4 / 45), "beta_half": (1 / 2, 3 / 8, 1 / 8, 35 / 128 - 9 / 64), "beta_2_1": (2 / 3, 1 / 2, 1 / 18, 1 / 12)}


@pytest.mark.parametrize("dist", sorted(MOMENTS))
def test_65536_drawn_times_stay_inside_and_have_the_right_moments(dist):
    n = 65536
    eng = _small()
    x = np.zeros((n, 2, 3), np.float32)
    t = eng.interpolate(x, x, t_distr=dist, seed=9, center="none")["t"]
    ref = vn.draw_t(dist, 9, 0, 0, n)
    assert (t > 0).all() and (t < 1).all()
    assert (np.abs(t - ref) <= np.spacing(ref)).all() and (dist != "uniform" or np.array_equal(t, ref))
    m1, m2, v1, v2 = MOMENTS[dist]
    t64 = t.astype(np.float64)
    assert abs(t64.mean() - m1) < 5 * np.sqrt(v1 / n)
    assert abs((t64 ** 2).mean() - m2) < 5 * np.sqrt(v2 / n)


# ------------------------------------------------------------------------------------------------ 6. determinism and splitting
def _six(g):
    ti = pkg()
    A = int(g["A"])
    return ti.synthetic.molecule_coords(6, A, seed=31), ti.synthetic.molecule_coords(6, A, seed=32), ti.synthetic.ambient_cond(6, A)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_same_call_twice_is_identical(precision):
    for name, case in (("vloss_ambient", "sig_sum"), ("vloss_latent_multi", "beta"), ("vloss_adw_h64", "standard")):
        eng, call, interp, s, g, c = _setup(name, case, precision)
        kw = dict(seed=4, draw=1, tbins=5, returns=("t", "z", "xt", "b"))
        r1, r2 = call(**kw), call(**kw)
        assert r1["mean"] == r2["mean"]
        for k in r1:
            if isinstance(r1[k], np.ndarray):
                assert np.array_equal(r1[k], r2[k]), (name, k)


PARTS = [(slice(0, 1), 0), (slice(1, 3), 1), (slice(3, 6), 3)]


def _split_runs(eng, x0, x1, cond, center):
    run = lambda sl, off: eng.velocity_loss(x0[sl], x1[sl], cond[sl], gamma="brownian", a=0.9, center=center, seed=8, draw=2, traj_offset=off,
                                            returns=("t", "z", "xt"))
    whole, split = run(slice(0, 6), 0), [run(sl, off) for sl, off in PARTS]
    return whole, {k: np.concatenate([p[k] for p in split], axis=1 if k == "xt" else 0) for k in ("loss", "t", "z", "xt")}


@pytest.mark.parametrize("precision", PRECISIONS)
def test_split_draws_batch_centre_and_adw(precision):
    """Six in one call against calls of 1, 2 and 3 with traj_offset 0, 1, 3.  The draws t, z are bit for bit the same whatever the
    centring; adw (NONE) also in the loss.  BATCH: the centre is the call's, so the split changes the states the drift is evaluated
    at -- asserted, so that the default is not mistaken for split-invariant (MOLECULE and NONE give the same states either way).  The
    cPaiNN drift itself is invariant under translations, so the LOSS moves with the centre only through round-off."""
    eng, call, interp, s, g, c = _setup("vloss_ambient", "brownian", precision)
    x0, x1, cond = _six(g)
    for center in ("molecule", "none", "batch"):
        whole, split = _split_runs(eng, x0, x1, cond, center)
        assert np.array_equal(whole["t"], split["t"]) and np.array_equal(whole["z"], split["z"])
        if center != "batch":
            assert np.array_equal(whole["xt"], split["xt"])
    assert np.abs(whole["xt"] - split["xt"]).max() > 1e-3 and not np.array_equal(whole["loss"], split["loss"])             # BATCH
    ea, _, _, sa, ga, _ = _setup("vloss_adw_h64", "standard", precision)
    b0, b1 = ga["beta0"].astype(np.float32), ga["beta1"].astype(np.float32)
    run = lambda sl, off: ea.velocity_loss(ga["x0"][sl], ga["x1"][sl], b0[sl], b1[sl], a=0.9, seed=8, draw=2, traj_offset=off, returns=("t", "z"))
    whole = run(slice(0, 6), 0)
    split = [run(sl, off) for sl, off in PARTS]
    for k in ("loss", "t", "z"):
        assert np.array_equal(whole[k], np.concatenate([p[k] for p in split])), k


@pytest.mark.parametrize("center", ["molecule", "none"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_split_loss_of_the_fixture_species_bit_for_bit(precision, center):
    """MOLECULE / NONE on the ambient fixture's species (A 6, complete graph): loss, t and z of six in one call against calls of 1, 2
    and 3 with traj_offset 0, 1, 3, bit for bit.  This species has no layout with one molecule per row group (30 edges, fewer than two
    row blocks: pinning 'latency' gives the packed layout), where a molecule's per-atom sums follow its slot in its group; the call lays
    its batch out with molecule b at slot (traj_offset + b) mod G, so the split does not move it."""
    eng, call, interp, s, g, c = _setup("vloss_ambient", "brownian", precision)
    x0, x1, cond = _six(g)
    eng.set_template("latency")
    try:
        assert eng.template_for(12) == "throughput"
        whole, split = _split_runs(eng, x0, x1, cond, center)
    finally:
        eng.set_template("auto")
    for k in ("loss", "t", "z"):
        assert np.array_equal(whole[k], split[k]), k


@pytest.mark.parametrize("center", ["molecule", "none"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_split_loss_with_one_molecule_per_row_group(precision, center):
    """The same check on a species that has the layout with one molecule per row group (A 8, complete graph, layout pinned to
    'latency': the drift's own condition for a result that does not depend on the batch)."""
    ti = pkg()
    W, syn = ti.weights, ti.synthetic
    A = 8
    key = ("a8", precision)
    if key not in _ENGINES:
        src, dst, ety = syn.fully_connected_template(A)
        flat = W.flatten_state_dict(syn.painn_state_dict(W.AMBIENT, 32, 2, 25, 5), W.painn_param_spec(W.AMBIENT, 32, 2, 25))
        _ENGINES[key] = ti.engine.PainnEngine(W.AMBIENT, 32, 2, A, src, dst, ety, np.arange(A, dtype=np.int32), flat, precision=precision)
    eng = _ENGINES[key]
    eng.set_template("latency")
    assert eng.template_for(12) == "latency"
    x0, x1, cond = syn.molecule_coords(6, A, seed=31), syn.molecule_coords(6, A, seed=32), syn.ambient_cond(6, A)
    whole, split = _split_runs(eng, x0, x1, cond, center)
    for k in ("loss", "t", "z"):
        assert np.array_equal(whole[k], split[k]), k


# ------------------------------------------------------------------------------------------------ 7. edges
def _reduce_ok(r, x0, x1, s_kw, slack=2):
    l, mag, n_terms = vn.loss(x0, x1, r["t"], r.get("z"), r["b"][0], r["b"][1] if r["b"].shape[0] == 2 else None, **s_kw)
    assert np.isfinite(r["loss"]).all()
    assert (np.abs(r["loss"] - l) <= slack * n_terms * U * mag).all()


def test_one_molecule_and_two_atoms():
    eng, call, interp, s, g, c = _setup("vloss_ambient", "brownian")
    r = eng.velocity_loss(g["x0"][:1], g["x1"][:1], g["cond"][:1], gamma="brownian", a=0.9, seed=1, returns=("t", "z", "xt", "b"))
    assert r["loss"].shape == (1,) and r["xt"].shape == (2, 1, int(g["A"]), 3)
    _reduce_ok(r, g["x0"][:1], g["x1"][:1], dict(gamma_kind="brownian", a=0.9))
    ti = pkg()
    small = _small()
    x0, x1, cond = ti.synthetic.molecule_coords(3, 2, seed=1), ti.synthetic.molecule_coords(3, 2, seed=2), ti.synthetic.ambient_cond(3, 2)
    r = small.velocity_loss(x0, x1, cond, gamma="sin2", seed=1, returns=("t", "z", "xt", "b"))
    _reduce_ok(r, x0, x1, dict(gamma_kind="sin2"))
    xt64, S = vn.interpolate(x0, x1, r["t"], r["z"], gamma_kind="sin2", center="batch")
    assert (np.abs(r["xt"] - xt64.astype(np.float32)) <= 2.0 ** -23 * S).all()
    both = small.drift(r["xt"].reshape(6, 2, 3), np.tile(r["t"], 2), np.tile(cond, (2, 1, 1)))           # the 2B states as one plain drift call:
    assert rel_l2(r["b"].reshape(6, 2, 3), both) < 1e-6                                                   # the same up to the slots in the row groups


@pytest.mark.parametrize("precision", PRECISIONS)
def test_edge_mask_applies_to_both_halves(precision):
    eng, call, interp, s, g, c = _setup("vloss_ambient", "brownian", precision)
    B, A = g["x0"].shape[:2]
    mask = np.full((B, A), (1 << A) - 1, np.uint32)
    mask[1, 0] &= ~np.uint32(1 << 2); mask[1, 2] &= ~np.uint32(1 << 0)            # molecule 1 loses the pair (0, 2), molecule 3 the pair (1, 4)
    mask[3, 1] &= ~np.uint32(1 << 4); mask[3, 4] &= ~np.uint32(1 << 1)
    kw = dict(returns=("t", "z", "xt", "b"), **_given(s, c))
    plain = call(**kw)
    eng.set_edge_mask(np.full((B, A), (1 << A) - 1, np.uint32))
    try:
        ones = call(**kw)                                                        # every edge present: the masked path, nothing masked
        eng.set_edge_mask(mask)
        r = call(**kw)
        _reduce_ok(r, g["x0"], g["x1"], _vn_kw(s))
        for half in (0, 1):                                                      # the masked drift of each half, evaluated on its own
            assert np.array_equal(r["b"][half], eng.drift(r["xt"][half], r["t"], g["cond"]))
    finally:
        eng.set_edge_mask(None)
    assert np.array_equal(r["xt"], plain["xt"]) and rel_l2(ones["b"], plain["b"]) < 1e-5
    changed = r["loss"] != ones["loss"]
    assert changed[1] and changed[3] and not changed[[0, 2, 4]].any()
    assert (np.abs(r["loss"] - plain["loss"])[[1, 3]] > 1e-9).all()                # and differs from the unmasked loss


def test_brownian_near_the_end_is_finite():
    eng, call, interp, s, g, c = _setup("vloss_ambient", "brownian")
    t = np.full(g["x0"].shape[0], 1e-6, np.float32)
    r = call(t=t, z=c["z"], returns=("t", "z", "xt", "b"))
    _reduce_ok(r, g["x0"], g["x1"], _vn_kw(s))


def test_refusals_on_the_device():
    import torch
    ti = pkg()
    eng, call, interp, s, g, c = _setup("vloss_ambient", "brownian")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    t0 = np.asarray(c["t"]).copy()
    t0[0] = 0.0
    with pytest.raises(ti._lib.TiError) as ei:                                   # a device-memory t is not read on the host
        eng.velocity_loss(dev(g["x0"]), dev(g["x1"]), dev(g["cond"]), gamma="brownian", a=s["a"], t=dev(t0), z=dev(c["z"]))
    assert ei.value.code == ti._lib.TI_E_NAN and "molecule 0" in str(ei.value)
    r = eng.velocity_loss(dev(g["x0"]), dev(g["x1"]), dev(g["cond"]), gamma="brownian", a=s["a"], t=dev(c["t"]), z=dev(c["z"]))      # the device path itself
    assert np.array_equal(r["loss"].cpu().numpy(), call(**_given(s, c))["loss"])
    with pytest.raises(ti._lib.TiError) as ei:
        call(t=t0, z=c["z"])
    assert ei.value.code == ti._lib.TI_E_ARG
    eng.set_molecules(np.full(g["x0"].shape[0], int(g["A"]), np.int32))
    try:
        with pytest.raises(ti._lib.TiError) as ei:
            call(**_given(s, c))
        assert ei.value.code == ti._lib.TI_E_UNSUPPORTED
    finally:
        eng.set_molecules(None)
    with pytest.raises(ti._lib.TiError) as ei:
        call(kind="one_sided", t=c["t"], z=c["z"])
    assert ei.value.code == ti._lib.TI_E_ARG and "z must be NULL" in str(ei.value)


# ------------------------------------------------------------------------------------------------ 8. time profile
@pytest.mark.parametrize("n", [1, 7])
def test_time_profile(n):
    for name, case in (("vloss_ambient", "sin2"), ("vloss_adw_h64", "standard")):
        eng, call, interp, s, g, c = _setup(name, case)
        r = call(seed=2, tbins=n, returns=("t", "z", "b"))
        B = g["x0"].shape[0]
        ref = vn.time_bins(r["loss"], r["t"], n)
        assert r["tbins"].shape == (n, 2) and r["tbins"][:, 1].sum() == B
        assert np.array_equal(r["tbins"][:, 1], ref[:, 1])
        _, mag, n_terms = vn.loss(g["x0"], g["x1"], r["t"], r["z"], r["b"][0], r["b"][1], **_vn_kw(s))
        assert (np.abs(r["tbins"][:, 0] - ref[:, 0]) <= 2 * B * U * np.abs(r["loss"]).sum()).all()
        assert abs(r["tbins"][:, 0].sum() - r["loss"].sum()) <= 2 * (n_terms + B) * U * mag.sum()
    t = np.asarray([0.0, 1.0, 0.5, 1.0 / 7, 0.999], np.float32)                  # the ends: t = 1 goes to the last bin
    eng, call, interp, s, g, c = _setup("vloss_ambient", "sin2")
    r = call(t=t, z=c["z"], tbins=n)
    assert np.array_equal(r["tbins"][:, 1], vn.time_bins(r["loss"], t, n)[:, 1])


# ------------------------------------------------------------------------------------------------ 9. the number means something
def test_trained_checkpoint_scores_below_untrained_and_matches_the_reference():
    ti = pkg()
    ref = load_golden("vloss_adw_trained")
    n = int(ref["n"])
    x0 = ti.synthetic.adw_boltzmann(n, float(ref["beta0"]), seed=int(ref["seed_x0"])).astype(np.float32)
    x1 = ti.synthetic.adw_boltzmann(n, float(ref["beta1"]), seed=int(ref["seed_x1"])).astype(np.float32)
    b0, b1 = np.full(n, float(ref["beta0"]), np.float32), np.full(n, float(ref["beta1"]), np.float32)
    res = {}
    for tag, fixture in (("trained", "adw_trained_h64"), ("untrained", "adw_ctor_h64")):
        eng = _adw_ckpt(fixture)[0]
        r = eng.velocity_loss(x0, x1, b0, b1, a=float(ref["a"]), seed=int(ref["seed"]), draw=int(ref["draw"]))
        res[tag] = (r["mean"], r["loss"].std(ddof=1) / np.sqrt(n))
        print(f"{tag}: mean {r['mean']:.5f} sem {res[tag][1]:.5f}   reference {float(ref[tag + '_mean']):.5f} sem {float(ref[tag + '_sem']):.5f}")
    (mt, st), (mu, su) = res["trained"], res["untrained"]
    assert mt < mu - 5 * max(st, su)
    assert abs(mt - float(ref["trained_mean"])) < 5 * st


# ------------------------------------------------------------------------------------------------ 10. fp16 storage mode
def test_f16_storage_mode_runs():
    eng, call, interp, s, g, c = _setup("vloss_ambient", "brownian", "f16")
    r = call(returns=("b",), **_given(s, c))
    assert np.isfinite(r["loss"]).all() and np.isfinite(r["mean"])
    assert rel_l2(r["b"], _ref_b(s, c)) < 1e-2


# ------------------------------------------------------------------------------------------------ 11. driver
def test_score_checkpoints_picks_the_trained_one(tmp_path):
    ti = pkg()
    _, sd_t, H, nl = _adw_ckpt("adw_trained_h64")
    _, sd_u, H2, nl2 = _adw_ckpt("adw_ctor_h64")
    assert (H, nl) == (H2, nl2)
    n = 1024
    x0, x1 = ti.synthetic.adw_boltzmann(2 * n, 1.0, seed=5).astype(np.float32), ti.synthetic.adw_boltzmann(2 * n, 1.25, seed=6).astype(np.float32)
    pairs = [(x0[i * n:(i + 1) * n, None], x1[i * n:(i + 1) * n, None], np.full((n, 1), 1.0), np.full((n, 1), 1.25)) for i in range(2)]
    outs = []
    for run in range(2):
        cfg = types.SimpleNamespace(gamma="brownian", t_distr="uniform", interpolant_a=0.9, n_draws=2, tbins=4, seed=3,
                                    data_save_path=str(tmp_path / f"run{run}"), data_save_name="adw")
        b = ti.thermo.adw.FCNetMultiBeta(1, 1, H, nl)
        res = ti.drivers.score_checkpoints(cfg, b, pairs, [sd_u, sd_t])
        with np.load(os.path.join(cfg.data_save_path, "val_loss_adw.npz")) as f:
            outs.append({k: f[k] for k in f.files})
        assert int(res["best"]) == 1 and all(np.array_equal(res[k], outs[-1][k]) for k in res)
    assert outs[0]["mean"].shape == (2,) and outs[0]["tbins"].shape == (2, 4, 2) and (outs[0]["tbins"][:, :, 1].sum(axis=1) == 2 * 2 * n).all()
    assert outs[0]["mean"][1] < outs[0]["mean"][0] - 5 * outs[0]["sem"].max()
    for k in outs[0]:
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k
