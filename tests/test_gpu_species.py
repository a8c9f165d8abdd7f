"""GPU: mixed-species batches (include/ti_hip.h ti_painn_set_molecules) -- molecules of 5, 9 and 12 atoms in one call on a handle
whose template is the complete graph on 12 atoms, each with its own radius + bond graph and its own bond types.

Parity: every molecule against an fp64 PainnOracle built with its own A_b, graph and types (the pattern of test_gpu_mask_matrix.py).
Bars, copied from the masked tests of the same quantities: drift max(DRIFT_TOL, 3x the fp32 oracle's own distance to fp64)
(test_gpu_mask_matrix.py:120); JVP tangent the same (test_gpu_mask_matrix.py:235); exact divergence DIV_ATOL * (|div| + 1)
(test_gpu_mask_matrix.py:231); Heun rollout_dlogp 1e-4 rel-L2 on the displacement and 1e-4 * (max |dlogp| + 1)
(test_gpu_mask_matrix.py:237-238); batch-control dopri5 against oracle/ode.py odeint 20 * tol + 2e-5 * max |x| and at most 12
evaluations apart (test_gpu_solvers.py:49-50).  Bit-level conditions are array_equal.  The EM bars are not copied: no existing test
compares EM noise with oracle.normal entry by entry; they are derived from fp32 rounding in that test's docstring.
Needs a real MI355X: `pytest -m gpu`.
"""
import functools
import types

import numpy as np
import pytest

from conftest import pkg, rel_l2
from oracle import ode, oracle
from test_gpu_divergence import DIV_ATOL
from test_gpu_parity import DRIFT_TOL

pytestmark = pytest.mark.gpu

T = 0.37
N_ATOMS = np.array([5, 12, 9, 12, 5, 9], np.int32)
A, B = 12, 6


def mask_words(on):
    return (on.astype(np.uint64) << np.arange(on.shape[1], dtype=np.uint64)[None, :, None]).sum(axis=1).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _problem(variant, F, L):
    ti = pkg()
    syn, W = ti.synthetic, ti.weights
    rs = np.random.RandomState(100 * variant + F)
    x = (50.0 * rs.standard_normal((B, A, 3))).astype(np.float32)               # pads: junk the results must not depend on
    on = np.zeros((B, A, A), bool)
    pt = np.zeros((B, A, A), np.uint8)
    for b, n in enumerate(N_ATOMS):
        x[b, :n] = syn.molecule_coords(1, n, seed=7 * b + n)[0]
        d = np.linalg.norm(x[b, :n, None].astype(np.float64) - x[b, None, :n], axis=-1)
        off = ~np.eye(n, dtype=bool)
        on[b, :n, :n] = (d <= np.quantile(d[off], 0.6)) & off
        i = np.arange(n - 1)
        on[b, i, i + 1] = on[b, i + 1, i] = True
        pt[b, i, i + 1] = pt[b, i + 1, i] = (i + n) % 3 + 1                     # bond orders differ between the species
    src, dst, et = syn.fully_connected_template(A)
    cond = {0: syn.ambient_cond(B, A), 1: np.repeat(np.float32([300, 500, 800, 400, 1000, 600]), A).reshape(B, A, 1), 2: None}[variant]
    flat = W.flatten_state_dict(syn.painn_state_dict(variant, F, L, 25, seed=F + L + variant), W.painn_param_spec(variant, F, L, 25))
    return types.SimpleNamespace(variant=variant, F=F, L=L, x=x, cond=cond, on=on, pt=pt, mask=mask_words(on), src=src, dst=dst, et=et, flat=flat)


def engine(p, precision="f32", layout=None, molecules=True):
    ti = pkg()
    eng = ti.engine.PainnEngine(p.variant, p.F, p.L, A, p.src, p.dst, p.et, np.arange(A), p.flat, temp_length=100.0, precision=precision)
    if layout is not None:
        eng.set_template(layout)
    if molecules:
        eng.set_molecules(N_ATOMS, p.mask, p.pt)
    return eng


def own(p, b):
    """(oracle of molecule b alone: its A_b, graph and types; its coordinates [1, n, 3]; its cond)."""
    n = int(N_ATOMS[b])
    s, d = np.nonzero(p.on[b, :n, :n])
    orc = oracle.PainnOracle(p.variant, p.F, p.L, n, s, d, p.pt[b, s, d], np.arange(n), p.flat, temp_length=100.0)
    return orc, p.x[b:b + 1, :n], None if p.cond is None else p.cond[b:b + 1, :n]


@functools.lru_cache(maxsize=None)
def _refs(variant, F, L, what):
    p = _problem(variant, F, L)
    out = []
    for b in range(B):
        orc, xb, cb = own(p, b)
        if what == "drift":
            ref = orc.drift(xb, T, cb, precision=64)
            out.append((ref, rel_l2(orc.drift(xb, T, cb), ref)))
        elif what == "div":
            out.append(orc.drift_div(xb, T, cb, precision=64))
        elif what == "jvp":
            xd = _xdot()[b:b + 1, :N_ATOMS[b]]
            ref = orc.jvp(xb, xd, T, cb, precision=64)
            out.append((ref, rel_l2(orc.jvp(xb, xd, T, cb, precision=32)[1], ref[1])))
        else:
            out.append(orc.rollout_dlogp(xb, cb, _grid(), scheme="heun", precision=64))
    return out


def _xdot():
    return np.random.RandomState(7).standard_normal((B, A, 3)).astype(np.float32)


def _grid():
    return pkg().engine.time_grid(0.0, 1.0, 4)


CASES = ([(0, F, pr, lay) for F in (32, 128, 256) for pr in ("f32", "f16x2") for lay in ("throughput", "latency", "pair") if lay != "pair" or F <= 128]
         + [(v, 32, pr, "throughput") for v in (1, 2) for pr in ("f32", "f16x2")] + [(1, 128, "f16x2", "pair"), (2, 128, "f32", "latency")])
LAYERS = 2


# ------------------------------------------------------------------------------------------- 1. parity with the fp64 oracle
@pytest.mark.parametrize("variant,F,precision,layout", CASES)
def test_mixed_batch_vs_per_molecule_fp64_oracle(variant, F, precision, layout):
    p = _problem(variant, F, LAYERS)
    eng = engine(p, precision, layout)
    assert eng.template_for(B) == layout                     # symmetric masks and types: the pair layout is eligible
    got = eng.drift(p.x, T, p.cond)
    assert np.isfinite(got).all()
    for b, (ref, floor) in enumerate(_refs(variant, F, LAYERS, "drift")):
        n = N_ATOMS[b]
        err = rel_l2(got[b:b + 1, :n], ref)
        print(f"drift v{variant} F{F} {precision} {layout} mol {b}: {err:.3e} (floor {floor:.3e})")
        assert err < max(DRIFT_TOL, 3 * floor), (b, err, floor)
        assert (got[b, n:] == 0).all() and not np.signbit(got[b, n:]).any()          # pad drift: exactly +0
    np.testing.assert_array_equal(eng.drift(p.x, T, p.cond), got)
    if layout == "pair":                                     # the tangent entry points walk directed rows
        eng.close()
        return
    out, div = eng.drift_div(p.x, T, p.cond)
    _, tan = eng.jvp(p.x, _xdot(), T, p.cond)
    path, dl, _ = eng.rollout_dlogp(p.x, p.cond, _grid(), scheme="heun")
    for b in range(B):
        n = N_ATOMS[b]
        ro, rd = _refs(variant, F, LAYERS, "div")[b]
        print(f"div mol {b}: {div[b]:.6e} vs {rd[0]:.6e}")
        assert rel_l2(out[b:b + 1, :n], ro) < max(DRIFT_TOL, 3 * _refs(variant, F, LAYERS, "drift")[b][1]), b
        assert abs(div[b] - rd[0]) < DIV_ATOL * (abs(rd[0]) + 1.0), (b, div[b], rd[0])
        (rb, rt), floor = _refs(variant, F, LAYERS, "jvp")[b]
        err = rel_l2(tan[b:b + 1, :n], rt)
        print(f"jvp mol {b}: {err:.3e} (floor {floor:.3e})")
        assert err < max(DRIFT_TOL, 3 * floor), (b, err, floor)
        assert (tan[b, n:] == 0).all()
        rp, rdl, _ = _refs(variant, F, LAYERS, "heun")[b]
        assert rel_l2(path[:, b:b + 1, :n] - path[0, b:b + 1, :n], rp - rp[0]) < 1e-4, b
        assert np.abs(dl[:, b] - rdl[:, 0]).max() < 1e-4 * (np.abs(rdl).max() + 1.0), b
        np.testing.assert_array_equal(path[:, b, n:], np.broadcast_to(p.x[b, n:], path[:, b, n:].shape))       # pads: x0, unchanged
    eng.close()


# ------------------------------------------------------------------------------------------- 2. independence from pad inputs
def _variants_of_pads(p):
    """The problem's inputs with other pad contents: moved far, duplicated onto a real atom and onto each other, other cond."""
    real = np.arange(A)[None, :] < N_ATOMS[:, None]
    x2, x3 = p.x.copy(), p.x.copy()
    x2[~real] = -1e4
    for b, n in enumerate(N_ATOMS):
        x3[b, n:] = p.x[b, 0]                                # every pad on top of real atom 0 (and of the other pads)
    c2 = p.cond.copy()
    c2[~real] = 12345.0
    return real, [(x2, p.cond), (x3, c2)]


@pytest.mark.parametrize("precision,layout", [("f32", "throughput"), ("f16x2", "latency"), ("f16x2", "pair")])
def test_real_atom_results_do_not_depend_on_pad_inputs(precision, layout):
    ti = pkg()
    p = _problem(0, 128, LAYERS)
    eng = engine(p, precision, layout)
    real, others = _variants_of_pads(p)
    grid = ti.engine.time_grid(0.0, 1.0, 5)
    xdot = _xdot()

    def everything(x, cond, xd):
        r = {"drift": eng.drift(x, T, cond)}
        r["euler"], _ = eng.rollout(x, cond, grid, scheme="euler")
        r["em"], _ = eng.rollout(x, cond, grid, scheme="em", eps=0.01, seed=3, com_free_noise=True)
        r["dopri5"], nfe = eng.rollout(x, cond, grid, scheme="dopri5", rtol=1e-4, atol=1e-4)
        r["nfe"] = np.asarray(nfe)
        r["traj"], _ = eng.rollout(x, cond, grid, scheme="dopri5", rtol=1e-4, atol=1e-4, step_control="trajectory")
        r["counts"] = np.stack(eng.step_counts(B))
        if layout != "pair":
            _, r["tan"] = eng.jvp(x, xd, T, cond)
            _, r["div"] = eng.drift_div(x, T, cond)
            _, r["est"] = eng.drift_div_est(x, T, cond, n_probes=3, probe_seed=5, traj_offset=40)
            _, r["dl"], _ = eng.rollout_dlogp(x, cond, grid, scheme="dopri5", rtol=1e-4, atol=1e-4)
        return r

    base = everything(p.x, p.cond, xdot)
    assert all(np.isfinite(v).all() for v in base.values())
    for x, cond in others:
        xd = xdot.copy()
        xd[~real] = 77.0
        got = everything(x, cond, xd)
        for k, v in base.items():
            if v.ndim >= 3:                                   # [.., B, A, 3]: real atoms bit for bit, pads where the call's x0 has them
                np.testing.assert_array_equal(got[k][..., real, :], v[..., real, :], err_msg=k)
                if k in ("euler", "em", "dopri5", "traj"):
                    np.testing.assert_array_equal(got[k][..., ~real, :], np.broadcast_to(x[~real], got[k][..., ~real, :].shape), err_msg=k)
                else:
                    assert (got[k][..., ~real, :] == 0).all(), k
            else:
                np.testing.assert_array_equal(got[k], v, err_msg=k)
    eng.close()


# ------------------------------------------------------------------------------------------- 3. full molecules = set_edge_mask
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_all_atoms_real_and_no_types_gives_the_edge_mask_bits(precision):
    ti = pkg()
    p = _problem(0, 128, LAYERS)
    full = np.arange(A)[None, :] < N_ATOMS[:, None]
    mask = p.mask.copy()
    mask[1] = mask[3] = (1 << A) - 1                         # the two 12-atom molecules complete; the others keep their sub-graphs
    grid = ti.engine.time_grid(0.0, 1.0, 4)
    res = []
    for setter in ("mask", "molecules"):
        eng = engine(p, precision, "throughput", molecules=False)
        if setter == "mask":
            eng.set_edge_mask(mask)
        else:
            eng.set_molecules(np.full(B, A, np.int32), mask)
        r = [eng.drift(p.x, T, p.cond), *eng.drift_div(p.x, T, p.cond), *eng.drift_div_est(p.x, T, p.cond, n_probes=2, probe_seed=1)]
        r += [eng.rollout(p.x, p.cond, grid, scheme="em", eps=0.01, com_free_noise=True)[0],
              eng.rollout(p.x, p.cond, grid, scheme="dopri5")[0], eng.rollout(p.x, p.cond, grid, scheme="dopri5", step_control="trajectory")[0]]
        res.append(r)
        eng.close()
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)
    # and the later call replaces the earlier one completely: molecules, then a mask, is the mask alone
    eng = engine(p, precision, "throughput")
    eng.set_edge_mask(mask)
    np.testing.assert_array_equal(eng.drift(p.x, T, p.cond), res[0][0])
    eng.set_molecules(None)
    ref = engine(p, precision, "throughput", molecules=False)
    np.testing.assert_array_equal(eng.drift(p.x, T, p.cond), ref.drift(p.x, T, p.cond))
    assert full.sum() < B * A
    eng.close(); ref.close()


# ------------------------------------------------------------------------------------------- 4. a molecule in the mix = its species alone
@pytest.mark.parametrize("precision,layout", [("f32", "latency"), ("f16x2", "latency")])
def test_trajectory_dopri5_and_hutchinson_equal_the_species_alone(precision, layout):
    """On the latency layout (one molecule per group) a molecule's rows are the same wherever it sits in a batch, so its bits are.  The
    throughput and pair layouts pack G molecules into the row blocks of one group, and a molecule's per-atom sums run in the block
    order of its position in that group: there the species-alone batch equals the mix to fp32 round-off only (measured 1.1e-6
    absolute on the path, f32 throughput), as for any two batches that place a molecule differently."""
    ti = pkg()
    p = _problem(0, 128, LAYERS)
    eng = engine(p, precision, layout)
    grid = ti.engine.time_grid(0.0, 1.0, 5)
    tol = 1e-5
    path, dl, _ = eng.rollout_dlogp(p.x, p.cond, grid, scheme="dopri5", rtol=tol, atol=tol, step_control="trajectory")
    counts = np.stack(eng.step_counts(B))
    _, est = eng.drift_div_est(p.x, T, p.cond, n_probes=3, probe_seed=9, traj_offset=100)
    for n in (5, 9, 12):
        idx = np.nonzero(N_ATOMS == n)[0]
        eng.set_molecules(N_ATOMS[idx], p.mask[idx], p.pt[idx])                   # the same handle and layout, this species only
        assert eng.template_for(len(idx)) == layout
        pa, da, _ = eng.rollout_dlogp(p.x[idx], p.cond[idx], grid, scheme="dopri5", rtol=tol, atol=tol, step_control="trajectory")
        np.testing.assert_array_equal(pa, path[:, idx])
        np.testing.assert_array_equal(da, dl[:, idx])
        np.testing.assert_array_equal(np.stack(eng.step_counts(len(idx))), counts[:, idx])
        for j, b in enumerate(idx):                          # Hutchinson: the probes of global id traj_offset + b
            _, e1 = eng.drift_div_est(p.x[idx], T, p.cond[idx], n_probes=3, probe_seed=9, traj_offset=100 + int(b) - j)
            np.testing.assert_array_equal(e1[j], est[b])
    eng.close()


@pytest.mark.parametrize("precision,layout", [("f32", "throughput"), ("f16x2", "throughput"), ("f32", "pair"), ("f16x2", "pair")])
def test_trajectory_dopri5_and_hutchinson_equal_the_species_alone_on_packed_layouts(precision, layout):
    """The throughput and pair layouts pack G molecules into one row group, and there a molecule's bits follow its place in the group
    with or without masks (include/ti_hip.h).  So the species-alone batch keeps every molecule of the species at its index of the
    mix and fills the other indices with molecules of the same species: a batch that contains only that species, same template
    pinned, same B.  Path, dlogp, step counts and the Hutchinson estimate of the kept molecules must be those of the mix, bit for bit:
    nothing a molecule computes may depend on the species of its neighbours in the group.  (The pair layout has no tangent entry
    points: path and step counts only.)"""
    ti = pkg()
    p = _problem(0, 128, LAYERS)
    eng = engine(p, precision, layout)
    grid = ti.engine.time_grid(0.0, 1.0, 5)
    tol = 1e-5
    kw = dict(scheme="dopri5", rtol=tol, atol=tol, step_control="trajectory")
    directed = layout != "pair"

    def run(x, cond):
        if directed:
            path, dl, _ = eng.rollout_dlogp(x, cond, grid, **kw)
            est = eng.drift_div_est(x, T, cond, n_probes=3, probe_seed=9, traj_offset=100)[1]
        else:
            (path, _), dl, est = eng.rollout(x, cond, grid, **kw), None, None
        return path, dl, est, np.stack(eng.step_counts(B))

    path, dl, est, counts = run(p.x, p.cond)
    assert len(set(counts.sum(axis=0).tolist())) > 1         # the molecules really take different numbers of steps
    for n in (5, 9, 12):
        idx = np.nonzero(N_ATOMS == n)[0]
        fill = idx[np.arange(B) % len(idx)]
        fill[idx] = idx                                      # the species' molecules where the mix has them, copies of them elsewhere
        assert (N_ATOMS[fill] == n).all()
        eng.set_molecules(N_ATOMS[fill], p.mask[fill], p.pt[fill])
        assert eng.template_for(B) == layout
        pa, da, ea, ca = run(p.x[fill], p.cond[fill])
        np.testing.assert_array_equal(pa[:, idx], path[:, idx])
        np.testing.assert_array_equal(ca[:, idx], counts[:, idx])
        if directed:
            np.testing.assert_array_equal(da[:, idx], dl[:, idx])
            np.testing.assert_array_equal(ea[idx], est[idx])
    eng.close()


# ------------------------------------------------------------------------------------------- 5. batch-control dopri5: the real-entry norm
@pytest.mark.parametrize("tol", [1e-4, 1e-6])
def test_batch_dopri5_vs_restatement_on_the_flat_real_state(tol):
    p = _problem(0, 32, LAYERS)
    eng = engine(p, "f32", "throughput")
    grid = np.linspace(0.0, 1.0, 5).astype(np.float32)
    path, nfe = eng.rollout(p.x, p.cond, grid, scheme="dopri5", rtol=tol, atol=tol)
    owns = [own(p, b) for b in range(B)]
    cuts = np.concatenate([[0], np.cumsum(N_ATOMS)])

    def func(t, y):                                          # the reference's flat [N, 3] state: the molecules' real atoms, concatenated
        return [np.concatenate([orc.drift(y[0][None, cuts[b]:cuts[b + 1]], t, cb)[0] for b, (orc, _, cb) in enumerate(owns)])]

    flat0 = np.concatenate([xb[0] for _, xb, _ in owns])
    sol, nfe_ref = ode.odeint(func, [flat0], grid, "dopri5", tol, tol)
    got = np.concatenate([path[:, b, :N_ATOMS[b]] for b in range(B)], axis=1)
    print(f"dopri5 tol {tol}: max |diff| {np.abs(got - sol[0]).max():.3e}, nfe {nfe} vs {nfe_ref}")
    assert got.shape == sol[0].shape and (nfe - 2) % 6 == 0
    assert np.abs(got - sol[0]).max() < 20 * tol + 2e-5 * np.abs(flat0).max()
    assert abs(nfe - nfe_ref) <= 12
    eng.close()


# ------------------------------------------------------------------------------------------- 6. EM noise
def test_em_noise_on_real_atoms_only_and_com_over_real_atoms():
    """One EM step minus the Euler step on the same drift is fl(fl(x + dt b) + fl(sigma z)) - fl(x + dt b): sigma z up to one rounding
    of the sum (half an ulp of |x| + |sigma z|, 6e-8 relative) and of the product, plus a few ulp of the device's logf / sinf / cosf
    against the oracle's libm at |z| <= 5.  Bound per entry: 2e-6 (|x| + 1) / sigma; the centre of mass sums n such entries."""
    p = _problem(0, 32, LAYERS)
    eng = engine(p, "f32", "throughput")
    grid = np.float32([0.0, 0.25])
    eps, seed, off, step = 0.02, 11, 1000, 6
    sigma = np.sqrt(np.float32(2.0) * np.float32(eps) * np.float32(0.25))
    det, _ = eng.rollout(p.x, p.cond, grid, scheme="euler")
    for com in (False, True):
        em, _ = eng.rollout(p.x, p.cond, grid, scheme="em", eps=eps, seed=seed, traj_offset=off, step_offset=step, com_free_noise=com)
        z = (em[1].astype(np.float64) - det[1]) / float(sigma)
        for b, n in enumerate(N_ATOMS):
            want = np.array([oracle.normal(seed, off + b, step, c) for c in range(3 * n)]).reshape(n, 3)
            if com:
                want = want - want.mean(axis=0, keepdims=True)
                assert np.abs(z[b, :n].sum(axis=0)).max() < 1e-5 * n / float(sigma), b            # fp32 round-off of the n updates
            assert np.abs(z[b, :n] - want).max() < 2e-6 * (np.abs(det[1][b, :n]).max() + 1.0) / float(sigma), b
            np.testing.assert_array_equal(em[1][b, n:], p.x[b, n:])                              # pads: no noise, unmoved
    eng.close()


# ------------------------------------------------------------------------------------------- 7. the mirror classes
def test_mirror_classes_take_a_mixed_batch_in_flat_node_order():
    """Consistency only: the mirror classes hand back the engine's own bits in flat node order.  The independent checks of the Python
    layer (against the reference's modules and the per-molecule oracle, ambient and latent) are in test_gpu_species_golden.py."""
    ti = pkg()
    p = _problem(0, 32, LAYERS)
    amb = ti.thermo.ambient
    items = []
    for b, n in enumerate(N_ATOMS):
        s, d = np.nonzero(p.on[b, :n, :n])
        items.append(ti.data.make_batch("ambient", p.x[b:b + 1, :n], (s, d, p.pt[b, s, d]), T0=float(p.cond[b, 0, 0]), T1=float(p.cond[b, 0, 1])))
    batch = ti.data.concat_species_batches(items)
    N = int(N_ATOMS.sum())
    batch.x0 = np.concatenate([p.x[b, :n] for b, n in enumerate(N_ATOMS)])      # the engine run's coordinates, bit for bit (make_batch re-centres)
    batch.x = batch.x0.copy()
    net = amb.cPaiNN(n_features=32, score_layers=LAYERS, temp_length=100.0)
    spec = ti.weights.painn_param_spec(0, 32, LAYERS, 25)
    net.load_state_dict(ti.weights.unflatten(p.flat, spec))
    batch.t = np.full(N, T, np.float32)
    out = net(batch).output
    assert out.shape == (N, 3)
    eng = engine(p, "f32")
    ref = eng.drift(p.x, T, p.cond)
    np.testing.assert_array_equal(out, np.concatenate([ref[b, :n] for b, n in enumerate(N_ATOMS)]))
    div = amb.ODEWrapper.compute_divergence(net, batch)
    np.testing.assert_array_equal(div, eng.drift_div(p.x, T, p.cond)[1] * np.float32(amb.ODEWrapper.DIV_SCALE))
    integ = amb.MoleculeIntegrator(b=net, method="euler", n_step=4, return_dlogp=True)
    xts, dlogp, _ = integ._rollout(batch)
    assert xts.shape == (4, N, 3) and dlogp.shape == (4, B)
    eng.close()
