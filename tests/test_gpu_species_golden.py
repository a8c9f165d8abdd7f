"""GPU: the mirror classes on a mixed-species batch against the reference's own modules (tests/golden/make_golden_species.py:
species_ambient.npz, species_latent.npz -- the reference's graph construction per molecule, its cPaiNN / ODEWrapper on the collated
batch of three species, everything stored in the reference's flat node order).

Bars: those tests/test_gpu_edge_mask.py applies to mask_*.npz (test_mirror_classes_against_the_reference_on_finite_cutoff_graphs):
drift rel-L2 < DRIFT_TOL (line 52) and < TOL through the ODEWrapper (line 55), divergence DIV_ATOL * (|div| + 1) after removing
DIV_SCALE (line 59), Euler displacement rel-L2 < 2e-5 (line 63).  The per-molecule fp64 oracle is a second, independent yardstick
for what the fixtures do not hold (dlogp of a rollout): bars of test_gpu_edge_mask.py:305-306.
Needs a real MI355X: `pytest -m gpu`.
"""
import types

import numpy as np
import pytest

from conftest import load_golden, pkg, rel_l2
from oracle import oracle
from test_gpu_divergence import DIV_ATOL, TOL
from test_gpu_parity import DRIFT_TOL

pytestmark = pytest.mark.gpu


def golden_batch(g, t):
    """The fixture's collated reference batch (molecules of 3 species, flat node order) as the mirror classes read it, at time t."""
    N = g["x"].shape[0]
    b = types.SimpleNamespace(x=g["x"].copy(), x0=g["x"].copy(), edge_index=g["edge_index"], edge_type=g["edge_type"], batch=g["batch"],
                              t=np.full(N, t, np.float32))
    if int(g["variant"]) == 0:
        b.atoms, b.T0, b.T1 = g["atom_ids"], g["cond"][:, 0].copy(), g["cond"][:, 1].copy()
    else:
        b.atom_number, b.T = g["atom_ids"], g["cond"][:, 0].astype(np.int64)
    return b


def _net(g, precision):
    ti = pkg()
    variant, F, L = (int(g[k]) for k in ("variant", "F", "L"))
    mod = ti.thermo.ambient if variant == 0 else ti.thermo.latent
    net = mod.cPaiNN(n_features=F, score_layers=L, temp_length=float(g["temp_length"]), temperatures=list(g["temperatures"]))
    net.precision = precision
    net.load_state_dict(ti.synthetic.painn_state_dict(variant, F, L, 25, int(g["seed"])))
    return mod, net


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("name", ["species_ambient", "species_latent"])
def test_mirror_classes_against_the_reference_on_a_mixed_species_batch(name, precision):
    ti = pkg()
    g = load_golden(name)
    mod, net = _net(g, precision)
    n_atoms, N = g["n_atoms"], g["x"].shape[0]
    sb = ti.thermo._molecule.split_species_batch(golden_batch(g, 0.0), net.ATOM_KEY)
    assert sb.n_atoms is not None and len(set(n_atoms.tolist())) == 3 and (sb.n_atoms == n_atoms).all()          # the mixed path
    for i, t in enumerate(g["ts"]):
        out = np.asarray(net(golden_batch(g, float(t))).output)
        err = rel_l2(out, g[f"drift_{i}"])
        print(f"{name} {precision} drift t={t}: {err:.3e}")
        assert out.shape == (N, 3) and err < DRIFT_TOL, (i, err)
        gb = golden_batch(g, float(t))
        b = np.asarray(mod.ODEWrapper(net)(np.float32(t), gb.x0, gb))                # the integrator's right-hand side
        assert b.shape == (N, 3) and rel_l2(b, g[f"drift_{i}"]) < TOL
    scale = mod.ODEWrapper.DIV_SCALE
    div = np.asarray(mod.ODEWrapper.compute_divergence(net, golden_batch(g, float(g["div_t"])))) / scale
    ref = g["div"].astype(np.float64) / scale
    print(f"{name} {precision} div: {div} vs {ref}")
    assert div.shape == ref.shape and (np.abs(div - ref) < DIV_ATOL * (np.abs(ref) + 1.0)).all(), (div, ref)
    integ = mod.MoleculeIntegrator(net, method="euler", n_step=len(g["traj_grid"]))
    path = np.asarray(integ.rollout(golden_batch(g, 0.0))[0])
    ref = g["traj_euler"]
    err = rel_l2(path - path[0], ref - ref[0])
    print(f"{name} {precision} euler: {err:.3e}")
    assert path.shape == ref.shape and err < 2e-5, err


@pytest.mark.parametrize("name", ["species_ambient", "species_latent"])
def test_mirror_rollout_with_dlogp_against_the_per_molecule_oracle(name):
    """MoleculeIntegrator with return_dlogp on the mixed batch: path in flat node order and dlogp [B] against one fp64 PainnOracle per
    molecule (its own A_b, graph and types) with the module's DIV_SCALE / SCALE_DLOGP: a wrong unpad order, scale or cond padding
    fails here."""
    ti = pkg()
    g = load_golden(name)
    mod, net = _net(g, "f32")
    variant, F, L, B = (int(g[k]) for k in ("variant", "F", "L", "B"))
    flat = ti.weights.flatten_state_dict(ti.synthetic.painn_state_dict(variant, F, L, 25, int(g["seed"])), ti.weights.painn_param_spec(variant, F, L, 25))
    integ = mod.MoleculeIntegrator(net, method="euler", n_step=4, return_dlogp=True)
    xts, dl = (np.asarray(v) for v in integ.rollout(golden_batch(g, 0.0))[:2])
    N = g["x"].shape[0]
    assert xts.shape == (4, N, 3) and dl.shape == (4, B)
    grid = ti.engine.time_grid(0.0, 1.0, 4)
    first = np.concatenate([[0], np.cumsum(g["n_atoms"])])
    mol = g["batch"][g["edge_index"][0]]
    ds, so = integ.DIV_SCALE, integ.SCALE_DLOGP
    for b in range(B):
        n, lo = int(g["n_atoms"][b]), int(first[b])
        e = mol == b
        orc = oracle.PainnOracle(variant, F, L, n, g["edge_index"][0][e] - lo, g["edge_index"][1][e] - lo, g["edge_type"][e], np.arange(n), flat,
                                 temp_length=float(g["temp_length"]), temperatures=list(g["temperatures"]))
        cond = g["cond"][lo:lo + n][None].astype(np.float32)
        rp, rdl, _ = orc.rollout_dlogp(g["x"][lo:lo + n][None], cond, grid, scheme="euler", precision=64, div_scale=ds)
        got = xts[:, lo:lo + n]
        assert rel_l2(got - got[0], rp[:, 0] - rp[0, 0]) < 1e-4, b
        assert np.abs(dl[:, b] - rdl[:, 0] * so).max() < 1e-3 * (np.abs(rdl * so).max() + 1.0), b
