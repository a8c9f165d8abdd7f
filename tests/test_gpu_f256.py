"""GPU: the mdqm9 configs' width -- n_features 256, score_layers 5, 25 atoms (config/ambient/10506_settings_no_*.json,
config/latent/10506_latent_allTs_settings.json) -- at every F = 256 message-kernel instantiation, against plain fp64 references.

painn_edge_kernel<16, FIRST, LAST, PREC, 4, NS> (painn_edge_nb8.hip) exists for four layer positions: L = 1 is the only way to reach
(FIRST, LAST) = (true, true), L = 5 the only one to reach the middle layers (false, false), which are three of the shipped model's five
message launches.  NS = 2 or 4 follows the template's max_slots (painn_edge_kernel.hpp: launch_edge_nb): with 25 atoms every destination
atom has 24 incoming rows, so no 16-row block holds more than two destination atoms (NS = 2); with 7 atoms the runs are 6 rows long and
blocks hold up to four (NS = 4).  Checked here: the drift at every (L, precision, template, NS) against the fp64 oracle; every stage
tap in both fp32-grade precisions against the oracle and a reference fixture; the tangent kernels stage by stage; the shipped solver
settings (dopri5, rtol = atol = 1e-5, dlogp, shared and per-trajectory step control); and the full-occupancy race / first-touch
screens at one resident workgroup per CU.

Bars: DRIFT_TOL (1e-5 rel-L2) or 3x the fp32 oracle's own distance to fp64 where that is larger (as for the magnitude fixtures); the
fp16 storage mode F16_TOL (1e-2).
"""
import functools

import numpy as np
import pytest

from conftest import golden_weights, load_golden, pkg, rel_l2
from oracle import ode, oracle

pytestmark = pytest.mark.gpu

DRIFT_TOL = 1e-5
F16_TOL = 1e-2
DIV_ATOL = 2e-5
F = 256


def _weights(L, seed=F):
    ti = pkg()
    W = ti.weights
    return W.flatten_state_dict(ti.synthetic.painn_state_dict(W.AMBIENT, F, L, 25, seed=seed), W.painn_param_spec(W.AMBIENT, F, L, 25))


def _problem(L, A, B, seed=0):
    ti = pkg()
    src, dst, et = ti.synthetic.fully_connected_template(A)
    args = (ti.weights.AMBIENT, F, L, A, src, dst, et, np.arange(A), _weights(L))
    return args, ti.synthetic.molecule_coords(B, A, seed=seed + A), ti.synthetic.ambient_cond(B, A)


@functools.lru_cache(maxsize=None)
def _oracle_drift(L, A, B):
    """(x, cond, fp64 drift, fp32 oracle distance to it) of one synthetic problem: shared by the precision / template cases."""
    args, x, cond = _problem(L, A, B)
    orc = oracle.PainnOracle(*args, temp_length=100.0)
    ref = orc.drift(x, 0.37, cond, precision=64)
    return x, cond, ref, rel_l2(orc.drift(x, 0.37, cond), ref)


# ------------------------------------------------------------------------------------------- 1. instantiation matrix
@pytest.mark.parametrize("A,B", [(25, 3), (7, 5)], ids=["NS2", "NS4"])
@pytest.mark.parametrize("template", ["throughput", "latency"])
@pytest.mark.parametrize("precision", ["f32", "f16x2", "f16"])
@pytest.mark.parametrize("L", [1, 2, 5])
def test_f256_message_instantiations_vs_fp64_oracle(L, precision, template, A, B):
    ti = pkg()
    x, cond, ref, floor = _oracle_drift(L, A, B)
    args, _, _ = _problem(L, A, B)
    eng = ti.engine.PainnEngine(*args, temp_length=100.0, precision=precision)
    eng.set_template(template)
    assert eng.template_for(B) == template                  # a pinned layout that exists for this molecule, not a fall-back
    got = eng.drift(x, 0.37, cond)
    bar = F16_TOL if precision == "f16" else max(DRIFT_TOL, 3 * floor)
    err = rel_l2(got, ref)
    assert np.isfinite(got).all() and err < bar, (L, precision, template, A, err, bar)
    np.testing.assert_array_equal(eng.drift(x, 0.37, cond), got)
    eng.close()


# ------------------------------------------------------------------------------------------- 2. stage taps, both fp32-grade paths
def _stages(L):
    return [(0, "embed")] + [s for l in range(L) for s in ((1 + 2 * l, f"msg{l}"), (2 + 2 * l, f"upd{l}"))]


def _golden_pair(g, precision):
    ti = pkg()
    args = (int(g["variant"]), int(g["F"]), int(g["L"]), int(g["A"]), g["edge_src"], g["edge_dst"], g["edge_type"], g["atom_ids"], golden_weights(g))
    kw = dict(temp_length=float(g["temp_length"]), temperatures=g["temperatures"])
    return ti.engine.PainnEngine(*args, precision=precision, **kw), oracle.PainnOracle(*args, **kw)


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_f256_stage_taps_vs_oracle_and_reference(precision):
    """s, v, e after the embed stage and after every one of the five message / update blocks (ambient_f256_taps: 6 atoms, NS = 4)."""
    g = load_golden("ambient_f256_taps")
    eng, orc = _golden_pair(g, precision)
    B, A, L = int(g["B"]), int(g["A"]), int(g["L"])
    assert (int(g["F"]), L) == (F, 5)
    t = float(g["ts"][1])
    try:
        for stage, tag in _stages(L):
            eng.debug_tap(stage)
            eng.drift(g["x"], t, g["cond"])
            _, taps = orc.drift(g["x"], t, g["cond"], tap_stage=stage)
            s = eng.debug_read("s", B)
            assert rel_l2(s, taps["s"]) < DRIFT_TOL, (tag, "s")
            if tag == "embed":
                assert rel_l2(s.reshape(B * A, F), g["im::s_embed"]) < DRIFT_TOL
                continue
            v = eng.debug_read("v", B).transpose(0, 1, 3, 2)
            assert rel_l2(v, taps["v"]) < DRIFT_TOL, (tag, "v")
            assert rel_l2(v.reshape(B * A, F, 3), g[f"im::v_{tag}"]) < DRIFT_TOL, (tag, "v golden")
            assert rel_l2(s.reshape(B * A, F), g[f"im::s_{tag}"]) < DRIFT_TOL, (tag, "s golden")
            if tag.startswith("msg") and int(tag[3:]) < L - 1:
                e = eng.debug_read("e", B)
                assert rel_l2(e, taps["e"]) < DRIFT_TOL, (tag, "e")
                assert rel_l2(e.reshape(-1, F), g[f"im::e_{tag}"]) < DRIFT_TOL, (tag, "e golden")
    finally:
        eng.debug_tap(-1)
    assert rel_l2(eng.drift(g["x"], t, g["cond"]), g["drift_1"]) < DRIFT_TOL


# ------------------------------------------------------------------------------------------- 3. tangent kernels at L = 5
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_f256_jvp_stage_taps_vs_oracle(precision):
    """Forward-mode tangents (both builds of the NBK = 16 tangent kernels) after every block of the five-layer model, small molecule."""
    g = load_golden("ambient_f256_taps")
    eng, orc = _golden_pair(g, precision)
    B, L, t = int(g["B"]), int(g["L"]), float(g["ts"][1])
    xdot = np.random.RandomState(7).standard_normal(g["x"].shape).astype(np.float32)
    b, tan = eng.jvp(g["x"], xdot, t, g["cond"])
    rb, rtan = orc.jvp(g["x"], xdot, t, g["cond"], precision=64)
    assert rel_l2(b, rb) < DRIFT_TOL and rel_l2(tan, rtan) < DRIFT_TOL, (rel_l2(b, rb), rel_l2(tan, rtan))
    try:
        for stage, tag in _stages(L)[1:]:
            eng.debug_tap(stage)
            eng.jvp(g["x"], xdot, t, g["cond"])
            _, _, taps = orc.jvp(g["x"], xdot, t, g["cond"], tap_stage=stage)
            assert rel_l2(eng.debug_read("ts", B), taps["s"]) < DRIFT_TOL, (tag, "ts")
            assert rel_l2(eng.debug_read("tv", B).transpose(0, 1, 3, 2), taps["v"]) < DRIFT_TOL, (tag, "tv")
            if tag.startswith("msg") and int(tag[3:]) < L - 1:
                assert rel_l2(eng.debug_read("te", B), taps["e"]) < DRIFT_TOL, (tag, "te")
    finally:
        eng.debug_tap(-1)
    # divergence of the same molecules against the fp64 oracle's forward-mode trace
    _, div = eng.drift_div(g["x"], t, g["cond"])
    _, odiv = orc.drift_div(g["x"], t, g["cond"], precision=64)
    assert (np.abs(div - odiv) < DIV_ATOL * (np.abs(odiv) + 1.0)).all(), (div, odiv)


# ------------------------------------------------------------------------------------------- 4. shipped solver settings
def test_f256_dopri5_with_dlogp_vs_restatement():
    """rtol = atol = 1e-5 and return_dlogp (the ambient configs), shared step size: the library's dopri5 against the numpy
    restatement (oracle/ode.py) over the oracle's drift and exact divergence; bounds of test_gpu_solvers.test_dopri5_with_dlogp_and_reverse."""
    ti = pkg()
    args, x, cond = _problem(5, 5, 2)
    eng, orc = ti.engine.PainnEngine(*args, temp_length=100.0), oracle.PainnOracle(*args, temp_length=100.0)
    tol, scale = 1e-5, 1e-2

    def rhs(sign):
        def f(t, y):
            b, div = orc.drift_div(y[0], t, cond)
            return [sign * b, (-sign * scale * div).astype(np.float32)]
        return f

    for rev, grid in ((False, np.linspace(0, 1, 3)), (True, np.linspace(1, 0, 3))):
        grid = grid.astype(np.float32)
        path, dl, nfe = eng.rollout_dlogp(x, cond, grid, scheme="dopri5", rtol=tol, atol=tol, div_scale=scale, reverse_ode=rev)
        sol, nfe_ref = ode.odeint(rhs(-1.0 if rev else 1.0), [x, np.zeros(2, np.float32)], grid, "dopri5", tol, tol)
        assert np.abs(path - sol[0]).max() < 20 * tol and np.abs(dl - sol[1]).max() < 20 * tol * (np.abs(sol[1]).max() + 1), rev
        assert abs(nfe - nfe_ref) <= 12


def test_f256_trajectory_step_control_is_per_molecule():
    """step_control='trajectory' on the shipped model (L = 5, 25 atoms) with dlogp: every molecule's path, dlogp and step counts are
    bit for bit what a batch of that molecule alone gives, and what a permuted batch gives, under the layout the full batch uses."""
    ti = pkg()
    B = 4
    args, x, cond = _problem(5, 25, B, seed=3)
    x = np.ascontiguousarray(x * np.float32([0.6, 1.0, 1.7, 2.5])[:, None, None])         # different stiffness: different step sizes
    eng = ti.engine.PainnEngine(*args, temp_length=100.0, precision="f16x2")
    eng.set_template(eng.template_for(B))
    grid = np.linspace(0.0, 1.0, 3).astype(np.float32)

    def run(idx):
        path, dl, _ = eng.rollout_dlogp(x[idx], cond[idx], grid, scheme="dopri5", step_control="trajectory", rtol=1e-5, atol=1e-5,
                                        div_scale=1e-2, out_scale=1e2)
        return path, dl, np.stack(eng.step_counts(len(idx)))

    full = run(np.arange(B))
    assert np.isfinite(full[0]).all() and np.isfinite(full[1]).all()
    assert len(set(full[2].sum(axis=0).tolist())) > 1                                       # the molecules really took their own steps
    perm = np.array([2, 0, 3, 1])
    runs = [(run(perm), perm)] + [(run(np.array([i])), np.array([i])) for i in range(B)]
    for got, idx in runs:
        np.testing.assert_array_equal(got[0], full[0][:, idx])
        np.testing.assert_array_equal(got[1], full[1][:, idx])
        np.testing.assert_array_equal(got[2], full[2][:, idx])


# ------------------------------------------------------------------------------------------- 5. full occupancy at NB = 8
# 25 atoms = 600 directed rows = 37.5 row blocks: the throughput template packs G = 2 molecules per group (75 full blocks), so B molecules
# are B / 2 waves in B / 8 four-wave workgroups; the latency template gives every molecule P >= 2 waves of its own.  At F = 256 one
# workgroup is resident per CU (launch bounds of painn_edge_kernel for NBK = 16; 256 CUs): B = 8192 is >= 1024 workgroups per launch,
# four or more generations of workgroups replacing finished ones.
OCC_B = 8192


def _occupancy_problem():
    ti = pkg()
    args, _, _ = _problem(5, 25, 1)
    return args, ti.synthetic.molecule_coords(OCC_B, 25, seed=0), ti.synthetic.ambient_cond(OCC_B, 25)


@pytest.mark.parametrize("template", ["throughput", "latency"])
def test_f256_race_screen_full_occupancy(template):
    """Mirror of test_gpu_parity.test_painn_race_screen_full_occupancy at the mdqm9 width: repeated launches of the f32 and split-fp16
    builds agree molecule by molecule (independent instruction streams; an early fragment read shows up as a few wrong molecules)."""
    ti = pkg()
    args, x, cond = _occupancy_problem()
    outs = []
    for prec in ("f32", "f16x2"):
        eng = ti.engine.PainnEngine(*args, temp_length=100.0, precision=prec)
        eng.set_template(template)
        assert eng.template_for(OCC_B) == template
        outs += [eng.drift(x, 0.5, cond).reshape(OCC_B, -1) for _ in range(3)]
        eng.close()
    ref = outs[0]
    assert np.isfinite(ref).all()
    scale = np.linalg.norm(ref, axis=1)
    for o in outs[1:]:
        per_mol = np.linalg.norm(o - ref, axis=1) / scale
        assert per_mol.max() < 3e-5, f"{(per_mol >= 3e-5).sum()} molecules disagree, worst {per_mol.max():.2e}"


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("template", ["throughput", "latency"])
def test_f256_first_touch_accumulators_ignore_stale_contents(template, precision, monkeypatch):
    """Mirror of test_gpu_pair.test_first_touch_accumulators_ignore_stale_contents at F = 256, L = 5, 25 atoms: with the per-atom
    accumulators poisoned (NaN, 1e30) before every evaluation, the first-touch path returns exactly what the zeroing path
    (TI_ZERO_ACC=1) returns."""
    ti = pkg()
    args, x, cond = _occupancy_problem()

    def engine(zeroing):
        if zeroing:
            monkeypatch.setenv("TI_ZERO_ACC", "1")
        eng = ti.engine.PainnEngine(*args, temp_length=100.0, precision=precision)
        monkeypatch.delenv("TI_ZERO_ACC", raising=False)
        eng.set_template(template)
        assert eng.template_for(OCC_B) == template
        return eng

    eng = engine(True)
    ref = [eng.drift(x, 0.5, cond) for _ in range(2)]
    eng.close()
    assert np.isfinite(ref[0]).all()
    np.testing.assert_array_equal(ref[1], ref[0])
    eng = engine(False)
    for poison in (float("nan"), 1e30):
        for _ in range(2):                                   # the second call meets the first one's leftovers as well
            eng.debug_poison(OCC_B, poison)
            np.testing.assert_array_equal(eng.drift(x, 0.5, cond), ref[0])
    eng.close()
