"""Per-molecule edge sets on the MI355X (include/ti_hip.h ti_painn_set_edge_mask; the masked twins of the message kernels).

A batch whose molecules have different radius graphs (the reference's finite cutoff, mdqm9_ambient.py:160-170) runs on the superset
template with a per-molecule mask.  Every molecule of such a batch must be what the unchanged CPU oracle computes for that molecule
with its OWN template: drift, exact divergence and dlogp rollouts, ambient and latent, A in {7, 18, 25}, every directed layout and the
pair layout.  An all-ones mask must give the unmasked bits exactly; masked atoms with no incoming edge end with zero messages, not
stale accumulator contents; traj_offset shards reproduce the full batch; an asymmetric mask keeps off the pair layout.
Needs a real MI355X: `pytest -m gpu`.
"""
import os
import types

import numpy as np
import pytest

from conftest import load_golden, pkg, rel_l2
from oracle import oracle
from test_gpu_divergence import DIV_ATOL, TOL
from test_gpu_parity import DRIFT_TOL

pytestmark = pytest.mark.gpu


def golden_batch(g, t):
    """The fixture's collated reference batch (its own graph per molecule) as the mirror classes read it, at time t."""
    A, B = int(g["A"]), int(g["B"])
    x = g["x"].reshape(B * A, 3)
    b = types.SimpleNamespace(x=x.copy(), x0=x.copy(), edge_index=g["edge_index"], edge_type=g["edge_type"], batch=g["batch"],
                              t=np.full(B * A, t, np.float32))
    if int(g["variant"]) == 0:
        b.atoms, b.T0, b.T1 = g["atom_ids"], g["cond"][..., 0].reshape(-1), g["cond"][..., 1].reshape(-1)
    else:
        b.atom_number, b.T = g["atom_ids"], g["cond"][..., 0].reshape(-1).astype(np.int64)
    return b


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("name", ["mask_ambient", "mask_latent", "mask_ambient_f256", "mask_latent_f256"])
def test_mirror_classes_against_the_reference_on_finite_cutoff_graphs(name, precision):
    """tests/golden/make_golden_mask.py: the reference's own graph construction (radius graph per sample, bonds, coalesce) and its
    cPaiNN / ODEWrapper on a batch whose molecules keep 40-80 % of their pairs, one with an atom without incoming edges."""
    ti = pkg()
    g = load_golden(name)
    variant, F, L, A, B = (int(g[k]) for k in ("variant", "F", "L", "A", "B"))
    mod = ti.thermo.ambient if variant == 0 else ti.thermo.latent
    net = mod.cPaiNN(n_features=F, score_layers=L, temp_length=float(g["temp_length"]), temperatures=list(g["temperatures"]))
    net.precision = precision
    net.load_state_dict(ti.synthetic.painn_state_dict(variant, F, L, 25, int(g["seed"])))
    assert ti.thermo._molecule.split_graph_batch(golden_batch(g, 0.0), net.ATOM_KEY)[-1] is not None      # the masked path
    for i, t in enumerate(g["ts"]):
        out = np.asarray(net(golden_batch(g, float(t))).output).reshape(B, A, 3)
        assert rel_l2(out, g[f"drift_{i}"]) < DRIFT_TOL, (i, rel_l2(out, g[f"drift_{i}"]))
        gb = golden_batch(g, float(t))
        b = np.asarray(mod.ODEWrapper(net)(np.float32(t), gb.x0, gb))                # the integrator's right-hand side
        assert rel_l2(b.reshape(B, A, 3), g[f"drift_{i}"]) < TOL
    scale = mod.ODEWrapper.DIV_SCALE
    div = np.asarray(mod.ODEWrapper.compute_divergence(net, golden_batch(g, float(g["div_t"])))) / scale
    ref = g["div"].astype(np.float64) / scale
    assert (np.abs(div - ref) < DIV_ATOL * (np.abs(ref) + 1.0)).all(), (div, ref)
    integ = mod.MoleculeIntegrator(net, method="euler", n_step=len(g["traj_grid"]))
    path = np.asarray(integ.rollout(golden_batch(g, 0.0))[0]).reshape(-1, B, A, 3)
    ref = g["traj_euler"]
    assert rel_l2(path - path[0], ref - ref[0]) < 2e-5


def bonds(A):
    """Chain bonds 0 - 1 - ... - (A - 2), both directions, types 1..3; atom A - 1 has no bond."""
    i = np.arange(A - 2)
    bi = np.stack([np.concatenate([i, i + 1]), np.concatenate([i + 1, i])])
    return bi, np.concatenate([i % 3 + 1, i % 3 + 1])


def case(A, B, variant=0, F=64, L=3, seed=0, keep=0.6):
    """Coordinates, per-molecule radius + bond graphs (about `keep` of the pairs; molecule 0's atom A - 1 far away: no incoming edge),
    the reference-shaped batch, weights, conditioning."""
    ti = pkg()
    syn, W, d = ti.synthetic, ti.weights, ti.data
    x = syn.molecule_coords(B, A, seed=seed)
    x[0, A - 1] += 25.0
    x = (x - x.mean(axis=1, keepdims=True)).astype(np.float32)
    dist = np.linalg.norm(x[:, :, None] - x[:, None, :], axis=-1)
    cutoff = float(np.quantile(dist[1:][:, ~np.eye(A, dtype=bool)], keep))
    bi, bt = bonds(A)
    tpls = [d.build_edge_template(x[b], cutoff, bi, bt) for b in range(B)]
    cond = [syn.ambient_cond(B, A), syn.latent_cond(B, A, 500.0), None][variant]
    kw = dict(T0=cond[0, 0, 0], T1=cond[:, 0, 1]) if variant == 0 else dict(T=500)
    batch = d.make_batch("ambient" if variant == 0 else "latent", x, tpls, **kw)
    flat = W.flatten_state_dict(syn.painn_state_dict(variant, F, L, 25, seed=F + A), W.painn_param_spec(variant, F, L, 25))
    B_, A_, src, dst, et, ids, mask = ti.thermo._molecule.split_graph_batch(batch, "atoms" if variant == 0 else "atom_number")
    assert mask is not None and (B_, A_) == (B, A)
    return types.SimpleNamespace(A=A, B=B, F=F, L=L, variant=variant, x=x, tpls=tpls, cond=cond, batch=batch, flat=flat, src=src, dst=dst,
                                 et=et, mask=mask, temp_length=100.0 if variant == 0 else 75.0)


def engine(c, precision="f32", src=None, dst=None, et=None):
    ti = pkg()
    return ti.engine.PainnEngine(c.variant, c.F, c.L, c.A, c.src if src is None else src, c.dst if dst is None else dst,
                                 c.et if et is None else et, np.arange(c.A), c.flat, temp_length=c.temp_length, precision=precision)


def own_oracle(c, b):
    s, d, t = c.tpls[b]
    return oracle.PainnOracle(c.variant, c.F, c.L, c.A, s, d, t, np.arange(c.A), c.flat, temp_length=c.temp_length)


def cond_of(c, b):
    return None if c.cond is None else c.cond[b:b + 1]


@pytest.mark.parametrize("layout", ["throughput", "latency", "pair"])
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("A,variant", [(7, 0), (18, 0), (25, 1), (18, 1)])
def test_masked_drift_per_molecule_against_the_oracle(A, variant, precision, layout):
    c = case(A, 11, variant=variant)
    eng = engine(c, precision)
    eng.set_template(layout)
    eng.set_edge_mask(c.mask)
    if layout == "pair":
        assert eng.template_for(c.B) == "pair"                   # radius + bond graphs are symmetric
    got = eng.drift(c.x, 0.4, c.cond)
    assert np.isfinite(got).all()
    for b in range(c.B):
        ref = own_oracle(c, b).drift(c.x[b:b + 1], 0.4, cond_of(c, b), precision=64)
        assert rel_l2(got[b:b + 1], ref) < DRIFT_TOL, (b, len(c.tpls[b][0]))
    np.testing.assert_array_equal(eng.drift(c.x, 0.4, c.cond), got)              # deterministic


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("A,variant", [(7, 0), (18, 0), (25, 1)])
def test_masked_divergence_and_dlogp_rollout_per_molecule(A, variant, precision):
    c = case(A, 6, variant=variant)
    eng = engine(c, precision)
    eng.set_edge_mask(c.mask)
    out, div = eng.drift_div(c.x, 0.3, c.cond)
    grid = pkg().engine.time_grid(0.0, 1.0, 4)
    path, dl, _ = eng.rollout_dlogp(c.x, c.cond, grid, scheme="heun")
    for b in range(c.B):
        orc = own_oracle(c, b)
        ro, rd = orc.drift_div(c.x[b:b + 1], 0.3, cond_of(c, b), precision=64)
        assert rel_l2(out[b:b + 1], ro) < DRIFT_TOL
        assert abs(div[b] - rd[0]) < DIV_ATOL * (abs(rd[0]) + 1.0), (b, div[b], rd[0])
        rp, rdl, _ = orc.rollout_dlogp(c.x[b:b + 1], cond_of(c, b), grid, scheme="heun", precision=64)
        assert rel_l2(path[:, b:b + 1] - path[0, b:b + 1], rp - rp[0]) < 1e-4
        assert np.abs(dl[:, b] - rdl[:, 0]).max() < 1e-4 * (np.abs(rdl).max() + 1.0)


def test_f16_storage_mode_masked_matches_its_own_per_molecule_handles():
    c = case(18, 5)
    eng = engine(c, "f16")
    eng.set_edge_mask(c.mask)
    got = eng.drift(c.x, 0.5, c.cond)
    for b in range(c.B):
        alone = engine(c, "f16", *c.tpls[b]).drift(c.x[b:b + 1], 0.5, cond_of(c, b))
        ref = own_oracle(c, b).drift(c.x[b:b + 1], 0.5, cond_of(c, b), precision=64)
        assert rel_l2(got[b:b + 1], ref) < 3.0 * max(rel_l2(alone, ref), 1e-4), b          # the fp16 storage mode's own bar


@pytest.mark.parametrize("layout", ["throughput", "latency", "pair"])
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_all_ones_mask_equals_no_mask_bit_for_bit(layout, precision):
    ti = pkg()
    c = case(18, 10)
    ones = np.full((c.B, c.A), (1 << c.A) - 1, np.uint32)
    grid = ti.engine.time_grid(0.0, 1.0, 4)
    res = []
    for m in (None, ones):
        eng = engine(c, precision)
        eng.set_template(layout)
        eng.set_edge_mask(m)
        r = [eng.drift(c.x, 0.4, c.cond)]
        r += list(eng.drift_div(c.x[:10], 0.4, c.cond[:10]))
        r += list(eng.drift_div_est(c.x, 0.4, c.cond, n_probes=3, probe_seed=5))
        r.append(eng.rollout(c.x, c.cond, grid, scheme="em", eps=0.3, seed=2)[0])
        res.append(r)
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)


def test_hutchinson_molecule_in_a_masked_batch_equals_it_alone():
    c = case(18, 7)
    eng = engine(c, "f32")
    eng.set_edge_mask(c.mask)
    out, est = eng.drift_div_est(c.x, 0.6, c.cond, n_probes=4, probe_seed=9, traj_offset=100)
    for b in range(c.B):
        o1, e1 = engine(c, "f32", *c.tpls[b]).drift_div_est(c.x[b:b + 1], 0.6, cond_of(c, b), n_probes=4, probe_seed=9, traj_offset=100 + b)
        assert rel_l2(out[b:b + 1], o1) < 3e-6
        assert abs(est[b] - e1[0]) < 1e-5 * (abs(e1[0]) + 1.0), (b, est[b], e1[0])


def test_per_trajectory_dopri5_molecule_matches_its_run_alone():
    c = case(7, 5)
    grid = pkg().engine.time_grid(0.0, 1.0, 5)
    eng = engine(c, "f32")
    eng.set_edge_mask(c.mask)
    tol = 1e-5
    path, _ = eng.rollout(c.x, c.cond, grid, scheme="dopri5", rtol=tol, atol=tol, step_control="trajectory")
    for b in range(c.B):
        alone, _ = engine(c, "f32", *c.tpls[b]).rollout(c.x[b:b + 1], cond_of(c, b), grid, scheme="dopri5", rtol=tol, atol=tol,
                                                         step_control="trajectory")
        assert np.abs(path[:, b] - alone[:, 0]).max() < 20 * tol


@pytest.mark.parametrize("layout", ["throughput", "pair"])
def test_atoms_without_incoming_edges_get_zero_messages_not_poison(monkeypatch, layout):
    """Molecule 0's last atom has no edge in its radius graph: its masked first-touch sums must replace the poisoned accumulators with
    zeros, exactly like the zeroing path (TI_ZERO_ACC=1: memsets, adds only)."""
    c = case(18, 64)
    assert not any(c.tpls[0][1] == c.A - 1)

    def run(zeroing):
        if zeroing:
            monkeypatch.setenv("TI_ZERO_ACC", "1")
        eng = engine(c, "f16x2")
        monkeypatch.delenv("TI_ZERO_ACC", raising=False)
        eng.set_template(layout)
        eng.set_edge_mask(c.mask)
        outs = []
        for _ in range(2):
            if not zeroing:
                eng.debug_poison(c.B, float("nan"))
            outs.append(eng.drift(c.x, 0.5, c.cond))
        return outs

    ref = run(True)
    assert np.isfinite(ref[0]).all()
    for g in run(False):
        np.testing.assert_array_equal(g, ref[0])


def test_traj_offset_shards_reproduce_the_full_masked_batch():
    ti = pkg()
    c = case(18, 12)
    grid = ti.engine.time_grid(0.0, 1.0, 4)
    eng = engine(c, "f16x2")
    eng.set_template("throughput")
    eng.set_edge_mask(c.mask)
    full, _ = eng.rollout(c.x, c.cond, grid, scheme="em", eps=0.2, seed=4)
    parts = []
    for lo, hi in ((0, 8), (8, 12)):                       # shards of whole molecule groups, each with its slice of the mask
        eng.set_edge_mask(c.mask[lo:hi])
        parts.append(eng.rollout(c.x[lo:hi], c.cond[lo:hi], grid, scheme="em", eps=0.2, seed=4, traj_offset=lo)[0])
    np.testing.assert_array_equal(np.concatenate(parts, axis=1), full)


def test_asymmetric_mask_keeps_off_the_pair_layout():
    ti = pkg()
    c = case(18, 64)
    eng = engine(c, "f16x2")
    eng.set_edge_mask(c.mask)                                # radius + bond graphs: symmetric sets
    assert eng.template_for(65536) == "pair"                 # where the automatic choice takes pair rows (template_for: any B)
    eng.set_template("pair")
    assert eng.template_for(c.B) == "pair"
    eng.set_template("auto")
    asym = c.mask.copy()
    d, s = int(c.tpls[1][1][0]), int(c.tpls[1][0][0])
    asym[1, d] &= ~np.uint32(1 << s)                         # molecule 1: drop s -> d, keep d -> s
    eng.set_edge_mask(asym)
    assert eng.template_for(65536) != "pair"                 # the automatic choice keeps off them with an asymmetric mask
    layout = eng.template_for(c.B)
    assert layout != "pair"
    got = eng.drift(c.x, 0.5, c.cond)
    assert np.isfinite(got).all()
    ref = own_oracle(c, 1)
    s1, d1, t1 = c.tpls[1]
    keep = ~((s1 == s) & (d1 == d))
    orc = oracle.PainnOracle(0, c.F, c.L, c.A, s1[keep], d1[keep], t1[keep], np.arange(c.A), c.flat, temp_length=c.temp_length)
    assert rel_l2(got[1:2], orc.drift(c.x[1:2], 0.5, c.cond[1:2], precision=64)) < DRIFT_TOL       # the directed edge really is gone
    assert rel_l2(got[1:2], ref.drift(c.x[1:2], 0.5, c.cond[1:2], precision=64)) > 10 * DRIFT_TOL
    eng.set_template("pair")
    with pytest.raises(ti._lib.TiError) as e:
        eng.drift(c.x, 0.5, c.cond)
    assert e.value.code == ti._lib.TI_E_UNSUPPORTED
    with pytest.raises(ti._lib.TiError):
        eng.template_for(c.B)
    eng.set_template(layout)
    np.testing.assert_array_equal(eng.drift(c.x, 0.5, c.cond), got)
    with pytest.raises(ti._lib.TiError) as e:               # another B than the mask's
        eng.drift(c.x[:5], 0.5, c.cond[:5])
    assert e.value.code == ti._lib.TI_E_ARG
    eng.set_edge_mask(None)                                  # cleared: any B again
    eng.drift(c.x[:5], 0.5, c.cond[:5])


def test_mirror_classes_take_the_reference_finite_cutoff_batch():
    """cPaiNN.forward, ODEWrapper.compute_divergence and MoleculeIntegrator.rollout on the reference-shaped batch."""
    ti = pkg()
    amb = ti.thermo.ambient
    c = case(18, 6, F=64, L=3)
    net = amb.cPaiNN(n_features=c.F, score_layers=c.L, temp_length=100)
    net.load_state_dict(ti.synthetic.painn_state_dict(0, c.F, c.L, 25, seed=c.F + c.A))
    batch = c.batch
    batch.t = np.full(c.B * c.A, 0.4, np.float32)
    out = net(batch).output.reshape(c.B, c.A, 3)
    div = amb.ODEWrapper.compute_divergence(net, batch)
    integ = amb.MoleculeIntegrator(net, method="euler", n_step=4, return_dlogp=True)
    xts, dl, _, _ = integ.rollout(batch)
    grid = ti.engine.time_grid(0.0, 1.0, 4)
    for b in range(c.B):
        orc = own_oracle(c, b)
        assert rel_l2(out[b:b + 1], orc.drift(c.x[b:b + 1], 0.4, cond_of(c, b), precision=64)) < DRIFT_TOL
        _, rd = orc.drift_div(c.x[b:b + 1], 0.4, cond_of(c, b), precision=64)
        assert abs(div[b] - rd[0] * 1e-2) < 2e-5 * (abs(rd[0] * 1e-2) + 1.0)
        rp, rdl, _ = orc.rollout_dlogp(c.x[b:b + 1], cond_of(c, b), grid, scheme="euler", precision=64, div_scale=1e-2)
        got = np.asarray(xts).reshape(-1, c.B, c.A, 3)[:, b]
        assert rel_l2(got - got[0], rp[:, 0] - rp[0, 0]) < 1e-4
        assert np.abs(np.asarray(dl)[:, b] - rdl[:, 0] * 1e2).max() < 1e-3 * (np.abs(rdl * 1e2).max() + 1.0)


def test_sample_ambient_with_a_finite_cutoff_matches_per_molecule_runs(tmp_path):
    ti = pkg()
    d = ti.data
    A, F, L = 9, 64, 2
    traj = np.random.RandomState(1).standard_normal((8, 7, A, 3)) * np.linspace(0.4, 1.6, 7)[None, :, None, None]
    os.makedirs(tmp_path / "test")
    np.save(tmp_path / "test" / "00031.npy", traj)
    bi, bt = bonds(A)
    ds = d.MDQM9SamplerDataset("00031.npy", str(tmp_path), "test", T0=1000, T1=300, scale=False, cutoff=1.0, bond_index=bi, bonds=bt)
    b = ti.thermo.ambient.cPaiNN(n_features=F, score_layers=L, temp_length=100)
    sd = ti.synthetic.painn_state_dict(0, F, L, 25, 3)
    b.load_state_dict(sd)
    cfg = types.SimpleNamespace(seed=0, batch_size=4, n_steps=5, atol=1e-5, rtol=1e-5, return_dlogp=0, method="euler",
                                data_save_path=str(tmp_path / "out"), data_save_name="t")
    samples, _ = ti.drivers.sample_ambient(cfg, b, ds)
    flat = ti.weights.flatten_state_dict(sd, ti.weights.painn_param_spec(0, F, L, 25))
    order = np.random.RandomState(0).permutation(7)
    grid = ti.engine.time_grid(0, 1, 5)
    sizes = set()
    for k, i in enumerate(order):
        x0 = d._remove_com(ds.data[i:i + 1].astype(np.float32))
        s, t, e = ds.graph_of(i)
        sizes.add(len(s))
        orc = oracle.PainnOracle(0, F, L, A, s, t, e, np.arange(A), flat, temp_length=100.0)
        ref, _ = orc.rollout(x0, ti.synthetic.ambient_cond(1, A, 1000.0, (300.0,)), grid, scheme="euler", precision=64)
        assert rel_l2(samples[k], ref[:, 0]) < 1e-5, k
    assert len(sizes) > 1                                   # the frames really have different graphs
