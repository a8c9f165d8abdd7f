"""GPU: mixed-species batches beyond B = 6, A = 12 (tests/test_gpu_species.py) -- the ragged integrator kernels and the pad helpers at
the sizes where they take their other paths.

Problem: ambient variant, F = 32, L = 2, template A = 25 (complete graph).  Five molecule kinds with 1, 2, 21, 22 and 25 atoms: 3n = 3, 6,
63, 66, 75, so the cut between real and pad entries falls on both sides of lane 64 of the per-trajectory kernels, and one kind has no pads.
Every kind has its own radius + chain graph and bond types (the one-atom kind has no edge).  Molecule b of a batch is kind b % 5 -- no block
size of the helpers (4, 8, 64, 128, 256) divides that period -- and copies of a kind share coordinates, so one fp64 PainnOracle per kind
serves any B.  Pads hold junk in three input sets: 50 * randn, -1e4, and every pad on top of the molecule's atom 0.

Batch sizes: 261 (more than one 256-thread block, no multiple of 4 or 8), 35 (11 reduction blocks of 256 entries) and 3500
(3500 * 75 = 262 500 > 1024 * 256 entries: the second grid-stride trip of the partial sums).

Every bar is copied from the existing test of the same quantity or is a bit-level equality:
  drift, JVP tangent  max(DRIFT_TOL, 3 x the fp32 oracle's own distance to fp64)          test_gpu_species.py:120, 138
  exact divergence    DIV_ATOL * (|div| + 1)                                              test_gpu_species.py:134
  Hutchinson          EST_ATOL * (S + 1), S = (1/k) sum |eps_i (J eps)_i|                  test_gpu_hutchinson.py:64
  Heun rollout_dlogp  1e-4 rel-L2 on the displacement, 1e-4 * (max |dlogp| + 1)            test_gpu_species.py:141-142
  trajectory dopri5   path 20 tol + 2e-5 max |x|, dlogp 20 tol out_scale (max |ref| + 1),   test_gpu_traj_dopri5.py:147, 184-187
                      attempts within 2
  batch dopri5        20 tol + 2e-5 max |x|, evaluations within 12                         test_gpu_species.py:325-326
  EM noise            per entry 2e-6 (|x| + 1) / sigma, centre of mass 1e-5 n / sigma       test_gpu_species.py:348-349
The one-atom kind's fp64 drift, tangent and divergence are exactly 0 (asserted), so rel_l2 is undefined there: its drift and tangent must
stay below DRIFT_TOL x the largest max |ref| among the other kinds, its divergence below DIV_ATOL.
Needs a real MI355X: `pytest -m gpu`.
"""
import functools
import types

import numpy as np
import pytest

from conftest import pkg
from oracle import ode, oracle
from test_gpu_hutchinson import EST_ATOL
from test_gpu_species import DIV_ATOL, DRIFT_TOL, mask_words, rel_l2

pytestmark = pytest.mark.gpu

T = 0.37
A, F, LAYERS = 25, 32, 2
KINDS = np.array([1, 2, 21, 22, 25], np.int32)
NK = len(KINDS)
JUNK = ("randn", "far", "atom0")
DIV_SCALE, OUT_SCALE = 1e-2, 1e2                  # the ambient wrapper's factors (include/ti_hip.h ti_painn_rollout_dlogp)
D0_DIV_SCALE = 100.0                              # a dlogp segment whose d1 = |div| div_scale / atol dwarfs the coordinates' d0: 100 h0 binds


# ------------------------------------------------------------------------------------------- the problem
@functools.lru_cache(maxsize=None)
def kinds():
    """Per kind: coordinates [n, 3], edge set on[s, d] and bond types [n, n] built as test_gpu_species._problem builds them, cond (T0, T1), a
    tangent direction [n, 3]; and the flat weights."""
    ti = pkg()
    syn, W = ti.synthetic, ti.weights
    out = []
    for k, n in enumerate(KINDS):
        x = syn.molecule_coords(1, n, seed=7 * k + n)[0]
        on, pt = np.zeros((n, n), bool), np.zeros((n, n), np.uint8)
        if n > 1:
            d = np.linalg.norm(x[:, None].astype(np.float64) - x[None, :], axis=-1)
            off = ~np.eye(n, dtype=bool)
            on = (d <= np.quantile(d[off], 0.6)) & off
            i = np.arange(n - 1)
            on[i, i + 1] = on[i + 1, i] = True
            pt[i, i + 1] = pt[i + 1, i] = (i + n) % 3 + 1
        cond = np.float32([1000.0, syn.LADDER[k]])
        xdot = np.random.RandomState(70 + k).standard_normal((n, 3)).astype(np.float32)
        out.append(types.SimpleNamespace(n=int(n), x=x, on=on, pt=pt, cond=cond, xdot=xdot))
    flat = W.flatten_state_dict(syn.painn_state_dict(0, F, LAYERS, 25, seed=F + LAYERS), W.painn_param_spec(0, F, LAYERS, 25))
    return out, flat


@functools.lru_cache(maxsize=None)
def orc_of(k):
    ks, flat = kinds()
    s, d = np.nonzero(ks[k].on)
    return oracle.PainnOracle(0, F, LAYERS, ks[k].n, s, d, ks[k].pt[s, d], np.arange(ks[k].n), flat, temp_length=100.0)


def cond_of(k):
    ks, _ = kinds()
    return np.broadcast_to(ks[k].cond, (1, ks[k].n, 2)).copy()


def mix(B, junk="randn"):
    """A batch of B molecules, molecule b of kind b % 5, with one of the three pad contents (coordinates, cond and tangent direction)."""
    ks, flat = kinds()
    kind = np.arange(B) % NK
    n_atoms = KINDS[kind]
    real = np.arange(A)[None, :] < n_atoms[:, None]
    rs = np.random.RandomState(B)
    fill = {"randn": (50.0, 12345.0, 77.0), "far": (-1e4, 0.0, -3.0), "atom0": (0.0, -50.0, 1e3)}[junk]
    x = np.full((B, A, 3), fill[0], np.float32)
    if junk == "randn":
        x = (50.0 * rs.standard_normal((B, A, 3))).astype(np.float32)
    cond = np.full((B, A, 2), fill[1], np.float32)
    xdot = np.full((B, A, 3), fill[2], np.float32)
    on_k, pt_k = np.zeros((NK, A, A), bool), np.zeros((NK, A, A), np.uint8)
    for k, q in enumerate(ks):
        on_k[k, :q.n, :q.n], pt_k[k, :q.n, :q.n] = q.on, q.pt
        x[kind == k, :q.n], cond[kind == k, :q.n], xdot[kind == k, :q.n] = q.x, q.cond, q.xdot
        if junk == "atom0":
            x[kind == k, q.n:] = q.x[0]
    return types.SimpleNamespace(B=B, kind=kind, n_atoms=n_atoms, real=real, x=x, cond=cond, xdot=xdot, mask=mask_words(on_k)[kind], pt=pt_k[kind],
                                 flat=flat)


def engine(m, precision="f32", layout="throughput"):
    ti = pkg()
    eng = ti.engine.PainnEngine(0, F, LAYERS, A, *ti.synthetic.fully_connected_template(A), np.arange(A), m.flat, temp_length=100.0, precision=precision)
    eng.set_template(layout)
    eng.set_molecules(m.n_atoms, m.mask, m.pt)
    assert eng.template_for(m.B) == layout
    return eng


def heun_grid():
    return np.linspace(0.0, 1.0, 4).astype(np.float32)


@functools.lru_cache(maxsize=None)
def refs(what):
    """fp64 references, one per kind (computed once, never written to)."""
    ks, _ = kinds()
    out = []
    for k, q in enumerate(ks):
        orc, xb, cb = orc_of(k), q.x[None], cond_of(k)
        if what == "drift":
            ref = orc.drift(xb, T, cb, precision=64)
            out.append((ref, rel_l2(orc.drift(xb, T, cb), ref)))
        elif what == "div":
            out.append(orc.drift_div(xb, T, cb, precision=64)[1][0])
        elif what == "jvp":
            ref = orc.jvp(xb, q.xdot[None], T, cb, precision=64)[1]
            out.append((ref, rel_l2(orc.jvp(xb, q.xdot[None], T, cb, precision=32)[1], ref)))
        else:
            out.append(orc.rollout_dlogp(xb, cb, heun_grid(), scheme="heun", precision=64)[:2])
    if what in ("drift", "jvp"):                  # the one-atom kind: exactly 0 in fp64, so the others' magnitude sets its bar
        assert (out[0][0] == 0).all() and all(np.abs(r).max() > 0 for r, _ in out[1:])
    if what == "div":
        assert out[0] == 0.0
    return out


def check_field(got, m, what, tag):
    """got [B, A, 3] (drift or tangent) of the mix m against the per-kind fp64 references; pads exactly +0."""
    rf = refs(what)
    top = max(np.abs(r).max() for r, _ in rf[1:])
    for b in range(m.B):
        k, n = m.kind[b], m.n_atoms[b]
        ref, floor = rf[k]
        if k == 0:
            worst = np.abs(got[b, :n]).max()
            if b == 0:
                print(f"{what} {tag} one-atom kind: max |got| {worst:.3e} (bar {DRIFT_TOL * top:.3e})")
            assert worst <= DRIFT_TOL * top, (b, worst)
        else:
            err = rel_l2(got[b:b + 1, :n], ref)
            if b < NK:
                print(f"{what} {tag} kind {k}: {err:.3e} (floor {floor:.3e})")
            assert err < max(DRIFT_TOL, 3 * floor), (b, k, err, floor)
    assert (got[~m.real] == 0).all() and not np.signbit(got[~m.real]).any()


def check_div(div, m, tag):
    rd = refs("div")
    for b in range(m.B):
        r = rd[m.kind[b]]
        if b < NK:
            print(f"div {tag} kind {m.kind[b]}: {div[b]:.6e} vs {r:.6e}")
        assert abs(div[b] - r) < DIV_ATOL * (abs(r) + 1.0), (b, div[b], r)          # the one-atom kind: r = 0, |div| < DIV_ATOL


def probes(seed, traj0, m, k):
    """eps [B, k, A, 3] of include/ti_hip.h: real components from the host Philox normal, pad components 0"""
    eps = np.zeros((m.B, k, A * 3), np.float32)
    for b in range(m.B):
        for p in range(k):
            for i in range(3 * m.n_atoms[b]):
                eps[b, p, i] = 1.0 if oracle.normal(seed, traj0 + b, p, i) >= 0.0 else -1.0
    return eps.reshape(m.B, k, A, 3)


def check_est(est, m, seed, traj0, k, tag):
    """(1/k) sum_p eps_p^T (J eps_p) from fp64 oracle JVPs along the same probes (test_gpu_hutchinson.oracle_estimate, per kind)"""
    ks, _ = kinds()
    eps = probes(seed, traj0, m, k)
    for kk, q in enumerate(ks):
        idx = np.nonzero(m.kind == kk)[0]
        e = eps[idx][:, :, :q.n].reshape(len(idx) * k, q.n, 3)
        xb, cb = np.repeat(q.x[None], len(e), axis=0), np.repeat(cond_of(kk), len(e), axis=0)
        terms = (e.astype(np.float64) * orc_of(kk).jvp(xb, e, T, cb, precision=64)[1]).reshape(len(idx), k, -1)
        ref, S = terms.sum(axis=2).mean(axis=1), np.abs(terms).sum(axis=2).mean(axis=1)
        print(f"est {tag} kind {kk}: max |err| {np.abs(est[idx] - ref).max():.3e} (S up to {S.max():.3e})")
        assert (np.abs(est[idx] - ref) < EST_ATOL * (S + 1.0)).all(), (kk, est[idx], ref, S)


# ------------------------------------------------------------------------------------------- a. parity at B = 261
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("layout", ["throughput", "latency", "pair"])
def test_parity_at_261_vs_per_kind_fp64_oracle(layout, precision):
    m = mix(261)
    eng = engine(m, precision, layout)
    tag = f"{precision} {layout}"
    got = eng.drift(m.x, T, m.cond)
    assert np.isfinite(got).all()
    check_field(got, m, "drift", tag)
    same = [got]
    if layout != "pair":                                     # the tangent entry points walk directed rows
        out, div = eng.drift_div(m.x, T, m.cond)
        check_field(out, m, "drift", tag + " (drift_div)")
        check_div(div, m, tag)
        _, tan = eng.jvp(m.x, m.xdot, T, m.cond)
        check_field(tan, m, "jvp", tag)
        _, est = eng.drift_div_est(m.x, T, m.cond, n_probes=2, probe_seed=5, traj_offset=1000)
        check_est(est, m, 5, 1000, 2, tag)
        same += [out, div, tan]
    if layout == "latency":                                  # one molecule per row group: a kind's copies are the same bits anywhere
        for v in same:
            for k in range(NK):
                idx = np.nonzero(m.kind == k)[0]
                np.testing.assert_array_equal(v[idx], np.broadcast_to(v[idx[0]], v[idx].shape), err_msg=f"kind {k}")
    eng.close()


# ------------------------------------------------------------------------------------------- b. per-trajectory dopri5 vs the restatement
@functools.lru_cache(maxsize=None)
def traj_ref(k, dlogp, rev):
    """oracle/ode.py odeint on molecule kind k alone (the pattern of test_gpu_traj_dopri5.py:145, 182): (path, dlogp or None, attempts)"""
    ks, _ = kinds()
    orc, cb, tol = orc_of(k), cond_of(k), 1e-5
    grid = (np.linspace(1, 0, 4) if rev else np.linspace(0, 1, 4)).astype(np.float32)
    if not dlogp:                                            # a descending grid integrates the same field backwards (ode._ReverseFunc)
        sol, nfe = ode.odeint(lambda t, y: [orc.drift(y[0], t, cb)], [ks[k].x[None]], grid, "dopri5", tol, tol)
        return sol[0][:, 0], None, (nfe - 2) // 6
    sign = -1.0 if rev else 1.0

    def f(t, y):
        bb, div = orc.drift_div(y[0], t, cb)
        return [sign * bb, (-sign * DIV_SCALE * div).astype(np.float32)]

    sol, nfe = ode.odeint(f, [ks[k].x[None], np.zeros(1, np.float32)], grid, "dopri5", tol, tol)
    return sol[0][:, 0], sol[1][:, 0], (nfe - 2) // 6


@pytest.mark.parametrize("rev", [False, True])
@pytest.mark.parametrize("dlogp", [False, True])
def test_traj_dopri5_vs_restatement_per_kind(dlogp, rev):
    """Every molecule of a B = 35 mix against the restatement on its kind alone.  3n = 63 | 66 | 75: the real / pad cut of the lane-stride
    loops (ode_ragged_kernels.hip traj_norm_ragged, traj_init_ragged_kernel, traj_advance_ragged_kernel) falls before, inside and at the
    end of the second stripe.  The one-atom kind's drift is 0: Hairer's d1 < 1e-5 branch and the ratio == 0 growth."""
    m = mix(35)
    eng = engine(m)
    tol = 1e-5
    grid = (np.linspace(1, 0, 4) if rev else np.linspace(0, 1, 4)).astype(np.float32)
    kw = dict(scheme="dopri5", step_control="trajectory", rtol=tol, atol=tol)
    if dlogp:
        path, dl, nfe = eng.rollout_dlogp(m.x, m.cond, grid, reverse_ode=rev, div_scale=DIV_SCALE, out_scale=OUT_SCALE, **kw)
    else:
        (path, nfe), dl = eng.rollout(m.x, m.cond, grid, **kw), None
    acc, rej = eng.step_counts(m.B)
    att = acc + rej
    assert nfe == 2 + 6 * att.max()
    ref_att = np.zeros(m.B, np.int64)
    for b in range(m.B):
        k, n = m.kind[b], m.n_atoms[b]
        rp, rdl, ref_att[b] = traj_ref(k, dlogp, rev)
        err = np.abs(path[:, b, :n] - rp).max()
        bar = 20 * tol + 2e-5 * np.abs(m.x[b, :n]).max()
        if b < NK:
            print(f"traj dopri5 dlogp={dlogp} rev={rev} kind {k}: path {err:.3e} (bar {bar:.3e}), attempts {att[b]} vs {ref_att[b]}")
        assert err < bar, (b, k, err)
        if dlogp:
            e2 = np.abs(dl[:, b] - rdl * OUT_SCALE).max()
            if b < NK:
                print(f"    dlogp {e2:.3e} (bar {20 * tol * OUT_SCALE * (np.abs(rdl).max() + 1):.3e})")
            assert e2 < 20 * tol * OUT_SCALE * (np.abs(rdl).max() + 1), (b, k, e2)
        np.testing.assert_array_equal(path[:, b, n:], np.broadcast_to(m.x[b, n:], path[:, b, n:].shape))     # pads: x0 in every saved row
    assert np.abs(att - ref_att).max() <= 2, (att, ref_att)
    assert len(set(att[:NK].tolist())) > 1 and len(set(ref_att[:NK].tolist())) > 1, (att[:NK], ref_att[:NK])  # the kinds really differ
    np.testing.assert_array_equal(path[0], m.x)
    eng.close()


# ------------------------------------------------------------------------------------------- c. batch-control dopri5: the real-entry norm
@functools.lru_cache(maxsize=None)
def flat_ref(tol):
    """odeint on the flat 71-atom state of one period of five kinds (test_gpu_species.py
    test_batch_dopri5_vs_restatement_on_the_flat_real_state): the rms over r replicas of the period is the rms over the period."""
    ks, _ = kinds()
    cuts = np.concatenate([[0], np.cumsum(KINDS)])
    grid = np.linspace(0.0, 1.0, 5).astype(np.float32)

    def func(t, y):
        return [np.concatenate([orc_of(k).drift(y[0][None, cuts[k]:cuts[k + 1]], t, cond_of(k))[0] for k in range(NK)])]

    flat0 = np.concatenate([q.x for q in ks])
    sol, nfe = ode.odeint(func, [flat0], grid, "dopri5", tol, tol)
    return sol[0], nfe, cuts, np.abs(flat0).max()


@pytest.mark.parametrize("B,tol", [(35, 1e-4), (35, 1e-6), (3500, 1e-4)])
def test_batch_dopri5_norm_over_real_entries_in_many_blocks(B, tol):
    """B = 35: 2625 entries, 11 blocks of rk_ratio_partial_ragged / scaled_sq_partial_ragged (is_pad's i / m across block boundaries, the
    multi-block partial tree).  B = 3500: 262 500 entries, 1024 blocks and a second grid-stride trip.  Zero-drift pad entries that were
    merely counted would not move the path much, so the three pad-junk input sets must also give the same bits.  Pad entries have zero
    drift, so the only sum they can move is Hairer's d0, and d0 sets a step only where 100 h0 = d0 / d1 is below h1: never for the
    drift alone on this model (d0 / d1 = 12 .. 21 against h1 <= 0.5).  So a two-state run with a Hutchinson dlogp whose div_scale puts
    d1 four orders above d0 (D0_DIV_SCALE) rides along, bit for bit between the input sets: there every step follows d0."""
    sol, nfe_ref, cuts, xmax = flat_ref(tol)
    grid = np.linspace(0.0, 1.0, 5).astype(np.float32)
    base = None
    for junk in JUNK:
        m = mix(B, junk)
        eng = engine(m)
        path, nfe = eng.rollout(m.x, m.cond, grid, scheme="dopri5", rtol=tol, atol=tol)
        stiff = eng.rollout_dlogp_est(m.x, m.cond, grid, n_probes=1, probe_seed=5, scheme="dopri5", rtol=tol, atol=tol, div_scale=D0_DIV_SCALE)
        eng.close()
        np.testing.assert_array_equal(path[:, ~m.real], np.broadcast_to(m.x[~m.real], path[:, ~m.real].shape))        # pads: the call's x0
        if base is None:
            base = (path, nfe, m, stiff)
            assert (nfe - 2) % 6 == 0
            worst = max(np.abs(path[:, m.kind == k, :KINDS[k]] - sol[:, None, cuts[k]:cuts[k + 1]]).max() for k in range(NK))
            print(f"batch dopri5 B {B} tol {tol}: max |diff| over every replica {worst:.3e}, nfe {nfe} vs {nfe_ref}")
            assert worst < 20 * tol + 2e-5 * xmax
            assert abs(nfe - nfe_ref) <= 12
        else:
            assert nfe == base[1], (junk, nfe, base[1])
            np.testing.assert_array_equal(path[:, m.real], base[0][:, base[2].real], err_msg=junk)
            assert stiff[2] == base[3][2], (junk, stiff[2], base[3][2])
            np.testing.assert_array_equal(stiff[0][:, m.real], base[3][0][:, m.real], err_msg=junk + " (two-state run)")
            np.testing.assert_array_equal(stiff[1], base[3][1], err_msg=junk + " (two-state run, dlogp)")


# ------------------------------------------------------------------------------------------- d. independence from pad inputs at B = 261
@pytest.mark.parametrize("precision,layout", [("f32", "throughput"), ("f16x2", "latency"), ("f16x2", "pair")])
def test_real_atom_results_do_not_depend_on_pad_inputs_at_261(precision, layout):
    """everything() of test_gpu_species.test_real_atom_results_do_not_depend_on_pad_inputs over the three pad contents: park_pads,
    zero_pads, copy_pads, noise_ragged and div_reduce_ragged on more than one workgroup."""
    B = 261
    grid = np.linspace(0.0, 1.0, 5).astype(np.float32)
    eng = engine(mix(B), precision, layout)

    def everything(m):
        x, cond = m.x, m.cond
        r = {"drift": eng.drift(x, T, cond)}
        r["euler"], _ = eng.rollout(x, cond, grid, scheme="euler")
        r["em"], _ = eng.rollout(x, cond, grid, scheme="em", eps=0.01, seed=3, com_free_noise=True)
        r["dopri5"], nfe = eng.rollout(x, cond, grid, scheme="dopri5", rtol=1e-4, atol=1e-4)
        r["nfe"] = np.asarray(nfe)
        r["traj"], _ = eng.rollout(x, cond, grid, scheme="dopri5", rtol=1e-4, atol=1e-4, step_control="trajectory")
        r["counts"] = np.stack(eng.step_counts(B))
        if layout != "pair":
            _, r["tan"] = eng.jvp(x, m.xdot, T, cond)
            _, r["div"] = eng.drift_div(x, T, cond)
            _, r["est"] = eng.drift_div_est(x, T, cond, n_probes=3, probe_seed=5, traj_offset=40)
            _, r["dl"], _ = eng.rollout_dlogp(x, cond, grid, scheme="dopri5", rtol=1e-4, atol=1e-4)
            # Hairer's d0 sets a trajectory's first step only where d0 / d1 < h1 (see the batch-norm test): a two-state run with D0_DIV_SCALE
            r["traj2"], r["traj2_dl"], _ = eng.rollout_dlogp_est(x, cond, grid, n_probes=1, probe_seed=5, traj_offset=40, scheme="dopri5", rtol=1e-4,
                                                                 atol=1e-4, step_control="trajectory", div_scale=D0_DIV_SCALE)
            r["traj2_counts"] = np.stack(eng.step_counts(B))
        return r

    m0 = mix(B, JUNK[0])
    base = everything(m0)
    assert all(np.isfinite(v).all() for v in base.values())
    for junk in JUNK[1:]:
        m = mix(B, junk)
        got = everything(m)
        for k, v in base.items():
            if v.ndim >= 3:                                   # [.., B, A, 3]: real atoms bit for bit, pads where the call's x0 has them, or +0
                np.testing.assert_array_equal(got[k][..., m.real, :], v[..., m.real, :], err_msg=f"{junk} {k}")
                pads = got[k][..., ~m.real, :]
                if k in ("euler", "em", "dopri5", "traj", "traj2"):
                    np.testing.assert_array_equal(pads, np.broadcast_to(m.x[~m.real], pads.shape), err_msg=f"{junk} {k}")
                else:
                    assert (pads == 0).all() and not np.signbit(pads).any(), (junk, k)
            else:
                np.testing.assert_array_equal(got[k], v, err_msg=f"{junk} {k}")
    eng.close()


# ------------------------------------------------------------------------------------------- e. EM noise at B = 261
def test_em_noise_at_261_per_entry_and_com_over_real_atoms():
    """noise_ragged (128 threads per block) on three blocks: every real entry against oracle.normal(seed, traj_offset + b, step, c), the
    centre of mass over the n real atoms; bounds and their derivation: test_gpu_species.test_em_noise_on_real_atoms_only_and_com_over_real_atoms.
    The one-atom kind with com_free_noise: its only draw is its own centre of mass, z - z / 1 = 0 exactly, so the step is the Euler step."""
    m = mix(261)
    eng = engine(m)
    grid = np.float32([0.0, 0.25])
    eps, seed, off, step = 0.02, 11, 1000, 6
    sigma = float(np.sqrt(np.float32(2.0) * np.float32(eps) * np.float32(0.25)))
    det, _ = eng.rollout(m.x, m.cond, grid, scheme="euler")
    want_all = [np.array([oracle.normal(seed, off + b, step, c) for c in range(3 * n)]).reshape(n, 3) for b, n in enumerate(m.n_atoms)]
    for com in (False, True):
        em, _ = eng.rollout(m.x, m.cond, grid, scheme="em", eps=eps, seed=seed, traj_offset=off, step_offset=step, com_free_noise=com)
        z = (em[1].astype(np.float64) - det[1]) / sigma
        for b, n in enumerate(m.n_atoms):
            want = want_all[b]
            if com:
                want = want - want.mean(axis=0, keepdims=True)
                assert np.abs(z[b, :n].sum(axis=0)).max() < 1e-5 * n / sigma, b
                if n == 1:
                    np.testing.assert_array_equal(em[1][b], det[1][b])
            assert np.abs(z[b, :n] - want).max() < 2e-6 * (np.abs(det[1][b, :n]).max() + 1.0) / sigma, (b, com)
            np.testing.assert_array_equal(em[1][b, n:], m.x[b, n:])                                   # pads: no noise, unmoved
        if not com:
            assert np.abs(z[m.kind == 0, 0]).min() > 0                                                # without it the one-atom kind is kicked
    eng.close()


# ------------------------------------------------------------------------------------------- f. chunked tangent passes
def _budget_gb(D):
    """TI_JVP_WS_GB that makes a tangent pass with D directions per molecule hold exactly two molecules.  csrc/painn_host.hip: a pass holds
    floor(budget / (D * bytes)) molecules, rounded down to whole groups of G, with bytes = 4 (12 A F + rows F + 3 A) per virtual
    molecule and rows = P * nblk * 16 / G edge rows per molecule.  At A = 25 on the complete graph both directed layouts have G = 1
    (600 rows in 38 blocks waste 1.3 %, within the 2 % at which the throughput layout stops growing G; the latency layout is G = 1 by
    construction) and 600 <= rows <= 600 / 0.85 (the latency layout's padding limit).  So lo <= bytes <= hi with hi < 1.5 lo, and a
    budget of 2 D hi holds 2 molecules at hi and floor(2 hi / lo) = 2 at lo."""
    lo, hi = 4 * (12 * A * F + 600 * F + 3 * A), 4 * (12 * A * F + 705 * F + 3 * A)
    assert 2 * hi < 3 * lo
    gb = 2 * D * hi / 1e9
    assert gb >= 0.001                                       # the library's floor for the variable
    return repr(gb)


@pytest.mark.parametrize("precision,layout", [("f32", "throughput"), ("f32", "latency"), ("f16x2", "throughput")])
def test_chunked_tangent_passes_on_a_mixed_batch(monkeypatch, precision, layout):
    """B = 40 in passes of two molecules: b0 > 0 in painn_drift_div_dev / painn_drift_div_est_dev (the atom counts, masked rows and div_reduce_ragged
    at the chunk's offset, park_pads with rep = D on a chunk).  Whole groups per pass: the bits of the single-pass call."""
    m = mix(40)
    eng = engine(m, precision, layout)
    k = 4
    eng.profile(True)

    def run():
        r = {}
        eng.profile_read("painn_jvp_readout")
        _, r["div"] = eng.drift_div(m.x, T, m.cond)
        r["div_passes"] = eng.profile_read("painn_jvp_readout")[0]          # one tangent readout launch per pass (the library's own count)
        _, r["est"] = eng.drift_div_est(m.x, T, m.cond, n_probes=k, probe_seed=5, traj_offset=1000)
        r["est_passes"] = eng.profile_read("painn_jvp_readout")[0]
        r["path"], r["dl"], _ = eng.rollout_dlogp(m.x, m.cond, heun_grid(), scheme="heun")
        r["heun_passes"] = eng.profile_read("painn_jvp_readout")[0]
        return r

    monkeypatch.delenv("TI_JVP_WS_GB", raising=False)
    one = run()
    assert (one["div_passes"], one["est_passes"], one["heun_passes"]) == (1, 1, 6)
    monkeypatch.setenv("TI_JVP_WS_GB", _budget_gb(3 * A))
    many = run()
    monkeypatch.setenv("TI_JVP_WS_GB", _budget_gb(k))
    _, many["est"] = eng.drift_div_est(m.x, T, m.cond, n_probes=k, probe_seed=5, traj_offset=1000)
    many["est_passes"] = eng.profile_read("painn_jvp_readout")[0]
    print(f"passes {precision} {layout}: div {many['div_passes']}, est {many['est_passes']}, heun {many['heun_passes']}")
    assert (many["div_passes"], many["est_passes"], many["heun_passes"]) == (20, 20, 120)
    for key in ("div", "est", "path", "dl"):
        np.testing.assert_array_equal(many[key], one[key], err_msg=key)
    tag = f"{precision} {layout} chunked"
    check_div(many["div"], m, tag)
    check_est(many["est"], m, 5, 1000, k, tag)
    rh = refs("heun")
    for b in range(m.B):
        kk, n = m.kind[b], m.n_atoms[b]
        rp, rdl = rh[kk]
        if kk == 0:                                           # exactly 0 drift in fp64: no scale of its own, the other kinds' as for the drift
            top = max(np.abs(r[0] - r[0][0]).max() for r in rh[1:])
            assert (rp == rp[0]).all() and np.abs(many["path"][:, b, :n] - m.x[b, :n]).max() <= 1e-4 * top
        else:
            assert rel_l2(many["path"][:, b:b + 1, :n] - m.x[b:b + 1, :n], rp - rp[0]) < 1e-4, b
        assert np.abs(many["dl"][:, b] - rdl[:, 0]).max() < 1e-4 * (np.abs(rdl).max() + 1.0), b
        np.testing.assert_array_equal(many["path"][:, b, n:], np.broadcast_to(m.x[b, n:], many["path"][:, b, n:].shape))
    eng.close()


# ------------------------------------------------------------------------------------------- g. traj_offset shards
@pytest.mark.parametrize("precision,layout,cut", [("f32", "latency", 17), ("f16x2", "latency", 17), ("f32", "throughput", 32), ("f16x2", "pair", 32),
                                                  ("f32", "pair", 32)])
def test_traj_offset_shards_reproduce_the_full_mixed_batch(precision, layout, cut):
    """Two shards of a B = 48 mix, each with its slice of n_atoms, mask and types and with traj_offset: EM path, Hutchinson estimate,
    trajectory-dopri5 path and step counts of the full batch, bit for bit.  Latency layout (one molecule per group): any cut, here 17.
    Packed layouts: shards of whole groups (include/ti_hip.h ti_painn_set_molecules) -- 32 is a multiple of every group size the pair
    layout can take (1, 2, 4, 8) and of the throughput layout's (1 at A = 25, see _budget_gb), is not the midpoint, and starts the
    second shard on another kind than the batch starts on (32 % 5 = 2)."""
    m = mix(48)
    eng = engine(m, precision, layout)
    grid = np.linspace(0.0, 1.0, 4).astype(np.float32)
    directed = layout != "pair"

    def run(sl, off):
        x, cond = m.x[sl], m.cond[sl]
        B = len(x)
        r = {"em": eng.rollout(x, cond, grid, scheme="em", eps=0.2, seed=4, traj_offset=off, com_free_noise=True)[0]}
        r["traj"] = eng.rollout(x, cond, grid, scheme="dopri5", rtol=1e-5, atol=1e-5, step_control="trajectory")[0]
        r["counts"] = np.stack(eng.step_counts(B))
        if directed:
            r["est"] = eng.drift_div_est(x, T, cond, n_probes=3, probe_seed=9, traj_offset=100 + off)[1]
        return r

    full = run(slice(0, 48), 0)
    assert len(set(full["counts"].sum(axis=0).tolist())) > 1
    for sl in (slice(0, cut), slice(cut, 48)):
        eng.set_molecules(m.n_atoms[sl], m.mask[sl], m.pt[sl])
        assert eng.template_for(sl.stop - sl.start) == layout
        part = run(sl, sl.start)
        for key, v in part.items():
            np.testing.assert_array_equal(v, full[key][..., sl] if key in ("counts", "est") else full[key][:, sl], err_msg=f"{key} {sl}")
    eng.close()
