"""Cases of the tests of the molecule trainer on per-molecule graphs (ti_painn_train_set_graphs): the cell matrix with its graphs, the
reference fixtures as padded cases, the restatement's answer for either (tests/painn_train_graphs_torch.py), and what poisons a pad."""
from types import SimpleNamespace

import numpy as np
import torch

import painn_train_cases as pc
import painn_train_graphs_torch as pgt
from conftest import load_golden, pkg


def _random_graphs(rs, B, A, n_atoms, p=0.6):
    """Independent bits per direction (asymmetric sets), bits on pads left in (the library clears them), per-molecule types"""
    bits = rs.random_sample((B, A, A)) < p                                    # [b, d, s]
    bits &= ~np.eye(A, dtype=bool)
    mask = (bits * (np.uint64(1) << np.arange(A, dtype=np.uint64))).sum(axis=-1, dtype=np.uint64).astype(np.uint32)
    return mask, rs.randint(0, 4, (B, A, A)).astype(np.uint8)


def _graphs(cell, rs):
    """(n_atoms, mask, pair_type) of a cell by its rule"""
    A, B, rule = cell["A"], cell["B"], cell["rule"]
    n = np.asarray(cell["n_atoms"], np.int32)
    if rule == "random":              # asymmetric masks that differ between molecules, one real atom without a live incoming edge, own types
        mask, pt = _random_graphs(rs, B, A, n)
        mask[0, 1] = 0
        assert len({m.tobytes() for m in mask}) == B
        return n, mask, pt
    if rule == "bits31":              # A = 32: words in which bit 31 or bit 0 alone decides, random ones elsewhere, the template's types
        mask, _ = _random_graphs(rs, B, A, n, 0.5)
        mask[0, 3], mask[0, 4] = np.uint32(1 << 31), np.uint32(0x7fffffff) & ~np.uint32(1 << 4)
        mask[0, 5], mask[0, 6] = np.uint32(1), np.uint32(0xfffffffe) & ~np.uint32(1 << 6)
        mask[0, 31] = np.uint32(1)
        return n, mask, None
    if rule == "one_bit":             # every template edge but 1 -> 0 of molecule 0
        mask = np.full((B, A), 0xffffffff, np.uint32)
        mask[0, 0] &= ~np.uint32(1 << 1)
        return n, mask, None
    if rule == "tail":                # full graphs but for the short last molecules, which are masked too
        mask, pt = _random_graphs(rs, B, A, n)
        short = n < A
        mask[~short] = 0xffffffff
        return n, mask, (pt, short)
    raise KeyError(rule)


# The cells: the smallest shapes at which the twins can go wrong.  seed: of the inputs, chosen on the CPU so that the float32 restatement
# stays below a third of 1e-5 in every tensor (tests/test_painn_train_graphs_host.py); FLOAT32_DECIDES records what no seed of ten does.
#   standard / one_sided-*  F 32, L 2, A 4, B 3, atoms (4, 2, 3): asymmetric masks that differ between molecules (the minus half must
#                           find b = r % B), a real atom without a live incoming edge, per-molecule types; the one-sided loss on the
#                           multi-T latent variant with each centring
#   single     a molecule with one atom beside others: no live edge, a zero drift, no contribution to any gradient
#   bits31     A 32, B 2, L 1: bit 31 and bit 0 decide, one pad
#   f256       F 256, L 1, A 3, B 2: one pad, one cleared bit
#   slices     F 32, L 1, A 8, B 19, standard: 2 x 19 x 56 = 2128 edge rows against the slice of 2048, the short masked molecules 17 and
#              18 in the second slice
_C = lambda **kw: kw
CELLS = {
    "standard": _C(variant=0, F=32, L=2, A=4, B=3, n_atoms=(4, 2, 3), kind="standard", gamma="sin2", a=1.0, center="batch", seed=0, rule="random"),
    "one_sided-batch": _C(variant=1, F=32, L=2, A=4, B=3, n_atoms=(4, 2, 3), kind="one_sided", gamma="brownian", a=1.0, center="batch", seed=1, rule="random"),
    "one_sided-molecule": _C(variant=1, F=32, L=2, A=4, B=3, n_atoms=(4, 2, 3), kind="one_sided", gamma="brownian", a=1.0, center="molecule", seed=1, rule="random"),
    "one_sided-none": _C(variant=1, F=32, L=2, A=4, B=3, n_atoms=(4, 2, 3), kind="one_sided", gamma="brownian", a=1.0, center="none", seed=1, rule="random"),
    "single": _C(variant=0, F=32, L=2, A=4, B=3, n_atoms=(4, 1, 3), kind="standard", gamma="brownian", a=0.9, center="batch", seed=0, rule="random"),
    "bits31": _C(variant=2, F=32, L=1, A=32, B=2, n_atoms=(32, 31), kind="standard", gamma="brownian", a=0.9, center="molecule", seed=0, rule="bits31"),
    "f256": _C(variant=0, F=256, L=1, A=3, B=2, n_atoms=(3, 2), kind="standard", gamma="sin2", a=1.0, center="batch", seed=8, rule="one_bit"),
    "slices": _C(variant=0, F=32, L=1, A=8, B=19, n_atoms=(8,) * 17 + (5, 3), kind="standard", gamma="brownian", a=0.9, center="batch", seed=0, rule="tail"),
}
CELL_IDS = list(CELLS)
# {cell: {tensor: float32 distance}}: tensors for which no seed in 0..9 keeps the float32 restatement below a third of 1e-5; for them
# 3 x the float32 distance is the bar (as painn_train_cases.EDGE_FLOAT32_DECIDES, and by its rule for the spread between hosts: the
# record holds every tensor that came within EDGE_HOST_SPREAD of a third).  f256 has 10 node rows and products over K = 512 and 1024;
# seed 8 has the smallest worst distance of the ten, two tensors above a third, the distances dense just below it.
FLOAT32_DECIDES = {
    "f256": {
        "net.8.layers.1.v.linear.weight": 4.959e-06, "net.8.layers.0.w.mlp.0.weight": 3.374e-06, "net.8.layers.0.w.mlp.1.weight": 3.256e-06,
        "net.8.layers.0.w.mlp.4.weight": 3.209e-06, "net.8.layers.0.w.mlp.3.weight": 3.190e-06, "net.8.layers.0.phi.mlp.1.weight": 3.132e-06,
        "net.2.embedding.weight": 3.032e-06, "net.8.layers.1.u.linear.weight": 3.028e-06, "net.8.layers.0.w.mlp.6.weight": 2.939e-06,
        "net.8.layers.0.phi.mlp.0.weight": 2.875e-06, "net.8.layers.0.phi.mlp.3.weight": 2.831e-06, "net.8.layers.0.w.mlp.0.bias": 2.808e-06,
        "net.8.layers.0.phi.mlp.6.weight": 2.805e-06, "net.8.layers.2.V.linear.weight": 2.798e-06, "net.8.layers.0.w.mlp.1.bias": 2.771e-06,
        "net.8.layers.0.phi.mlp.0.bias": 2.739e-06, "net.8.layers.0.phi.mlp.1.bias": 2.733e-06},
}


def graph_case(name, seed=None):
    """A cell as a case of painn_train_cases.make_case's form on the full template, with n_atoms, mask, pair_type and N"""
    cell = CELLS[name]
    seed = cell["seed"] if seed is None else seed
    c = pc.make_case(cell["variant"], cell["F"], cell["L"], cell["A"], cell["B"], tpl="full", kind=cell["kind"], gamma=cell["gamma"], a=cell["a"],
                     center=cell["center"], seed=seed)
    n, mask, pt = _graphs(cell, np.random.RandomState(7000 + seed))
    if isinstance(pt, tuple):                                 # "tail": own types on the short molecules, the template's on the others
        own, short = pt
        A = cell["A"]
        tpl = np.zeros((A, A), np.uint8)
        tpl[c["model"]["src"], c["model"]["dst"]] = c["model"]["etype"]
        pt = np.where(short[:, None, None], own, tpl[None]).astype(np.uint8)
    c.update(n_atoms=n, mask=mask, pair_type=pt, N=int(n.sum()), name=name)
    return c


def fixture_case(name):
    """A reference fixture (tests/golden/make_golden_painn_train_graphs.py) as a padded case: the collated batch through the package's
    split_species_batch, on the fully connected template over the largest molecule"""
    ti = pkg()
    from importlib import import_module
    mol = import_module("thermodynamic-interpolation_amd.thermo._molecule")
    g = load_golden(name)
    variant, F, L, A, B = (int(g[k]) for k in ("variant", "F", "L", "A", "B"))
    n_atoms = g["n_atoms"]
    ids = np.concatenate([np.arange(n) for n in n_atoms]).astype(np.int64)
    batch = SimpleNamespace(atoms=ids, edge_index=g["edge_index"], edge_type=g["edge_type"], batch=g["batch"])
    sb = mol.split_species_batch(batch, "atoms")
    assert sb.A == A and sb.B == B and np.array_equal(sb.n_atoms, n_atoms)
    spec = ti.weights.painn_param_spec(variant, F, L, 25)
    flat = ti.weights.flatten_state_dict(ti.synthetic.painn_state_dict(variant, F, L, 25, int(g["seed"])), spec).astype(np.float64)
    kind = str(g["kind"])
    model = dict(variant=variant, F=F, L=L, src=sb.src, dst=sb.dst, etype=sb.etype, atom_ids=sb.atom_ids, temp_length=float(g["temp_length"]))
    c = dict(model=model, spec=spec, flat=flat, x0=sb.pad(g["x0"], 3), x1=sb.pad(g["x1"], 3), cond=sb.pad(g["cond"], g["cond"].shape[1]), t=g["t"],
             z=sb.pad(g["z"], 3) if kind == "standard" else None, center="batch", lk=dict(kind=kind, gamma=str(g["gamma"]), a=float(g["a"])), A=A, B=B,
             n_atoms=sb.n_atoms, mask=sb.mask, pair_type=sb.pair_type, N=int(n_atoms.sum()), name=name)
    c["g64"] = {k: g[f"g64::{k}"] for k, _ in spec}
    c["d32"] = {k: float(g[f"d32::{k}"]) for k, _ in spec}
    for k in ("rows64", "mean64", "rows32", "mean32"):
        c[k] = g[k]
    return c


def states(c):
    return pgt.states(c["x0"], c["x1"], c["t"], c["z"], c["n_atoms"], center=c["center"], **c["lk"])


def reference(c, dtype=torch.float64):
    """-> (loss rows [B], mean, {key: gradient}, drift [halves, B, A, 3]) of the restatement in `dtype`"""
    torch.set_num_threads(8)
    return pgt.grads(c["flat"], c["spec"], c["model"], c["n_atoms"], c["mask"], c["pair_type"], states(c), c["x0"], c["x1"], c["t"], c["z"], c["cond"],
                     dtype=dtype, **c["lk"])


def make_trainer(c, **kw):
    """The device trainer of a case with its graphs set"""
    tr = pc.make_trainer(c, **kw)
    tr.set_graphs(c["n_atoms"], c["mask"], c["pair_type"])
    return tr


def poisoned(c, value):
    """The case with every pad entry of x0, x1, cond and z set to `value`"""
    pad = np.arange(c["A"])[None, :] >= np.asarray(c["n_atoms"])[:, None]
    out = dict(c)
    for k in ("x0", "x1", "cond", "z"):
        if c[k] is not None:
            v = c[k].copy()
            v[pad] = value
            out[k] = v
    return out


def zero_pads(c, v):
    """v [B, A, ..] with 0 on the pad atoms"""
    pad = np.arange(c["A"])[None, :] >= np.asarray(c["n_atoms"])[:, None]
    v = np.array(v, copy=True)
    v[pad] = 0
    return v
