"""Cases of the molecule-trainer tests: synthetic weights, templates and batches at any shape, the restatement's answer for them
(tests/painn_train_torch.py), and the per-tensor comparison both test files use."""
import numpy as np
import torch

import painn_train_torch as ptt
import vloss_numpy as vn
from conftest import pkg


def sparse_template(A):
    """Unequal in-degrees, atom 0 without incoming edges, edge types 0..3 all present (A >= 3)."""
    pairs = [(0, 1), (0, 2)]
    for i in range(1, A - 1):
        pairs += [(i, i + 1), (i + 1, i)]
    pairs += [(1, A - 1)] if A > 3 else []
    pairs = sorted(set(pairs))
    src, dst = (np.asarray(v, np.int32) for v in zip(*pairs))
    return src, dst, (np.arange(len(pairs)) % 4).astype(np.int32)


def make_case(variant, F, L, A, B, tpl="full", kind="standard", gamma="brownian", a=1.0, center="batch", seed=0, repeat_ids=False, x_scale=1.0):
    ti = pkg()
    syn, W = ti.synthetic, ti.weights
    rs = np.random.RandomState(1000 + seed)
    spec = W.painn_param_spec(variant, F, L, 25)
    flat = W.flatten_state_dict(syn.painn_state_dict(variant, F, L, 25, seed), spec).astype(np.float64)
    if tpl == "full":
        src, dst, et = syn.fully_connected_template(A)
        et = ((et + np.arange(et.size)) % 4).astype(np.int32) if A > 2 else et
    else:
        src, dst, et = sparse_template(A)
    ids = (np.arange(A) % 2 + 3 if repeat_ids else (np.arange(A) * 3 + 1) % 25).astype(np.int32)
    # the target set displaced against the base by a fixed per-atom pattern: the residual of the untrained drift keeps one sign per
    # atom across the rows, so that a bias gradient is not the remainder of a random walk
    shape = rs.standard_normal((A, 3))
    x0 = (x_scale * (0.3 * rs.standard_normal((B, A, 3)) + 0.5 * shape)).astype(np.float32)
    x1 = (x_scale * (0.3 * rs.standard_normal((B, A, 3)) + 1.5 * shape)).astype(np.float32)
    ncond = W.N_COND[variant]
    cond = None
    if ncond:
        cond = np.empty((B, A, ncond), np.float32)
        cond[..., 0] = 1000.0 if ncond == 2 else 300.0 + 100.0 * (np.arange(B) % 8)[:, None]
        if ncond == 2:
            cond[..., 1] = 300.0 + 100.0 * (np.arange(B) % 6)[:, None]
    t = (0.1 + 0.8 * rs.random_sample(B)).astype(np.float32)
    z = rs.standard_normal((B, A, 3)).astype(np.float32) if kind == "standard" else None
    model = dict(variant=variant, F=F, L=L, src=src, dst=dst, etype=et, atom_ids=ids)
    return dict(model=model, spec=spec, flat=flat, x0=x0, x1=x1, cond=cond, t=t, z=z, center=center, lk=dict(kind=kind, gamma=gamma, a=a),
                A=A, B=B)


def states(c):
    """xt [halves, B, A, 3] as the interpolate kernels give it: the fp64 expression rounded to float32 once"""
    xt, _ = vn.interpolate(c["x0"], c["x1"], c["t"], c["z"], kind=c["lk"]["kind"], gamma_kind=c["lk"]["gamma"], a=c["lk"]["a"], center=c["center"])
    return xt.astype(np.float32)


def reference(c, dtype=torch.float64):
    """-> (loss rows [B], mean, {key: gradient}) of the restatement in `dtype`"""
    torch.set_num_threads(8)
    return ptt.grads(c["flat"], c["spec"], c["model"], states(c), c["x0"], c["x1"], c["t"], c["z"], c["cond"], dtype=dtype, **c["lk"])


def make_trainer(c, **kw):
    ti = pkg()
    m = c["model"]
    if "temp_length" in m:
        kw = dict(temp_length=m["temp_length"], **kw)
    return ti.engine.PainnTrainer(m["variant"], m["F"], m["L"], c["A"], m["src"], m["dst"], m["etype"], m["atom_ids"], c["flat"], **kw)


FIXTURE_CASES = [("painn_train_ambient", g) for g in ("brownian", "sin2", "sig_sum")] + [("painn_train_latent", td) for td in ("uniform", "beta")]


def fixture_case(name, case):
    """A reference fixture (tests/golden/make_golden_painn_train.py) as a case of make_case's form, with the reference's answers:
    g64 {key: gradient}, d32 {key: the float32 model's distance}, rows64, mean64, rows32, mean32"""
    from conftest import load_golden
    ti = pkg()
    g = load_golden(name)
    side = load_golden(f"{name}_{case}") if name == "painn_train_ambient" and case != "brownian" else g
    variant, F, L, A, B = (int(g[k]) for k in ("variant", "F", "L", "A", "B"))
    spec = ti.weights.painn_param_spec(variant, F, L, 25)
    flat = ti.weights.flatten_state_dict(ti.synthetic.painn_state_dict(variant, F, L, 25, int(g["seed"])), spec).astype(np.float64)
    ambient = name == "painn_train_ambient"
    lk = dict(kind="standard", gamma=case, a=float(g["a"][list(g["cases"]).index(case)])) if ambient else dict(kind="one_sided", gamma="brownian", a=1.0)
    model = dict(variant=variant, F=F, L=L, src=g["edge_src"], dst=g["edge_dst"], etype=g["edge_type"], atom_ids=g["atom_ids"],
                 temp_length=float(g["temp_length"]))
    pre = f"{case}::"
    c = dict(model=model, spec=spec, flat=flat, x0=g["x0"], x1=g["x1"], cond=g["cond"], t=g[pre + "t"], z=g[pre + "z"] if ambient else None,
             center="batch", lk=lk, A=A, B=B)
    c["g64"] = {k: side[f"{pre}g64::{k}"] for k, _ in spec}
    c["d32"] = {k: float(side[f"{pre}d32::{k}"]) for k, _ in spec}
    for k in ("rows64", "mean64", "rows32", "mean32"):
        c[k] = side[pre + k]
    return c


def call_kw(c):
    return dict(kind=c["lk"]["kind"], gamma=c["lk"]["gamma"], a=c["lk"]["a"], center=c["center"], t=c["t"], z=c["z"])


def split(flat, spec):
    out, o = {}, 0
    for k, shape in spec:
        n = int(np.prod(shape))
        out[k] = np.asarray(flat[o:o + n]).reshape(shape)
        o += n
    return out


def tensor_errors(got, ref64, ref32=None):
    """[(key, rel-L2 of got against ref64, bar)] with bar = max(1e-5, 3 x the float32 yardstick's own distance); tensors whose
    reference is all zero are checked to be exactly zero (err 0 or inf)."""
    rows = []
    for k, r in ref64.items():
        g = got[k]
        nr = np.linalg.norm(r)
        if nr == 0.0:
            rows.append((k, 0.0 if not np.any(g) else np.inf, 0.0))
            continue
        bar = 1e-5 if ref32 is None else max(1e-5, 3.0 * np.linalg.norm(ref32[k] - r) / nr)
        rows.append((k, float(np.linalg.norm(g - r) / nr), bar))
    return rows


def zero_violations(got, ref64):
    """The entries the reference leaves exactly zero that are not exactly zero in `got`: [(key, count)]"""
    out = []
    for k, r in ref64.items():
        n = int(np.count_nonzero(got[k][r == 0.0]))
        if n:
            out.append((k, n))
    return out


# The shape matrix of the GPU test: (variant, F, L, A, B, template, loss kind, gamma, a, centring, repeated atom ids).  Every variant,
# F = 32 / 64 and 128 once, L = 1..3, A in {2, 3, 7, 9}, B in {1, 5, 37}, both loss kinds, the three centrings, the sparse template,
# repeated ids.  The fourth cell has 2 x 37 x 72 = 5328 edge rows: three weight-gradient slices of 2048, the last one ragged.
# The last entry is the seed of the inputs, chosen on the CPU so that the plain float32 restatement stays below a third of 1e-5 in
# every tensor (tests/test_painn_train_host.py).  In the two cells of FLOAT32_DECIDES no seed of ten tried does: `v.linear.weight`
# sits at 3.5e-6 .. 8e-6 in float32 there (the derivative of ||vv|| divides by a norm that is small for some features, on few
# rows), so for that tensor the bar is 3 x the float32 distance and not the floor.
MATRIX = [
    (0, 32, 1, 2, 1, "full", "standard", "brownian", 0.9, "batch", False, 0),
    (1, 32, 2, 3, 5, "sparse", "one_sided", "brownian", 1.0, "molecule", False, 11),
    (2, 64, 3, 7, 5, "sparse", "standard", "sin2", 1.0, "none", True, 22),
    (0, 64, 2, 9, 37, "full", "standard", "sig_sum", 4.0, "batch", False, 13),
    (1, 128, 1, 3, 5, "full", "one_sided", "brownian", 1.0, "none", False, 14),
    (2, 32, 3, 9, 1, "full", "standard", "brownian", 0.9, "molecule", True, 5),
    (0, 32, 2, 7, 37, "sparse", "one_sided", "brownian", 1.0, "batch", False, 6),
]
FLOAT32_DECIDES = (2, 4)
MATRIX_IDS = ["-".join(str(v) for v in cell[:10]) for cell in MATRIX]


# The edge cells: the shapes the study trains (F = 128 / 256, L = 5, A = 18), the caps, and the row counts at which the trainer's
# tiling changes path.  Same layout as MATRIX, the same rule for the seed.  With R = halves x B molecules a call (halves = 2 for the
# standard loss, 1 for the one-sided), a cell has R A node rows, 3 R A vector rows and R E edge rows:
#   0  F = 256 at all: LayerNorm's fourth entry a lane, products with K = 1024 / 512 and N = 1280 / 768
#   1  the study's ambient model: L = 5 (`ge` chained through four layers), E = 306
#   2  F = 256 through five layers on the latent variant, R = 3
#   3  the atom cap: E = 992, in-degree 31, repeated atom ids
#   4  exact slice multiples: 2048 node rows, 6144 vector rows, 63 488 = 31 x 2048 edge rows; R = 64 = 4 x 16 table rounds
#   5  one row over: 2049 node rows, 6147 vector rows; 683 molecules through the table accumulators
#   6  R = 1, two node rows: one partial 16-row product tile, one table accumulator in use
#   7, 8  R = 16 and 17: the end of the first accumulator round and one molecule into the second
EDGE_MATRIX = [
    (0, 256, 1, 3, 2, "full", "standard", "sin2", 1.0, "molecule", False, 8),
    (0, 128, 5, 18, 2, "full", "standard", "sin2", 1.0, "batch", False, 9),
    (1, 256, 5, 18, 3, "full", "one_sided", "brownian", 1.0, "none", False, 7),
    (2, 64, 2, 32, 2, "full", "standard", "sig_sum", 4.0, "batch", True, 1),
    (0, 32, 1, 32, 32, "full", "standard", "brownian", 0.9, "molecule", False, 0),
    (1, 32, 1, 3, 683, "sparse", "one_sided", "brownian", 1.0, "batch", False, 0),
    (1, 32, 1, 2, 1, "full", "one_sided", "brownian", 1.0, "none", False, 0),
    (2, 32, 1, 3, 16, "sparse", "one_sided", "brownian", 1.0, "molecule", True, 0),
    (2, 32, 1, 3, 17, "sparse", "one_sided", "brownian", 1.0, "batch", False, 0),
]
EDGE_IDS = ["-".join(str(v) for v in cell[:10]) for cell in EDGE_MATRIX]
EDGE_EXACT, EDGE_ONE_OVER = 4, 5
# Edge cells in which no seed of ten (0..9) keeps every tensor's float32 distance below 1e-5 / 3; the kept seed is the one with the
# smallest worst distance.  Both are F = 256 cells with few rows (12 and 54 node rows; the float32 products run over K = 512 and
# 1024), and in both the distances lie densely around a third.  The float32 restatement does not give the same bits on every
# host: between an Intel Xeon and an AMD EPYC 9575F the distances of these tensors differ by up to 11 %.  So a cell's record is
# {tensor: the larger of the two hosts' distances} for every tensor that came within EDGE_HOST_SPREAD of a third on either host
# (above a third: 5 and 7 tensors of cell 0, 13 and 12 of cell 2).  For a tensor above a third 3 x its float32 distance is the bar.
# tests/test_painn_train_host.py asserts that nothing outside the record exceeds a third, that the record holds nothing far below
# it, and that every tensor stays below 1e-5.
EDGE_HOST_SPREAD = 1.25
EDGE_FLOAT32_DECIDES = {
    0: {
        "net.8.layers.1.v.linear.weight": 7.111e-06, "net.8.layers.0.w.mlp.0.weight": 3.865e-06,
        "net.8.layers.0.w.mlp.3.weight": 3.621e-06, "net.8.layers.0.w.mlp.1.weight": 3.566e-06,
        "net.8.layers.0.w.mlp.4.weight": 3.454e-06, "net.2.embedding.weight": 3.376e-06, "net.8.layers.0.phi.mlp.1.weight": 3.342e-06,
        "net.8.layers.0.phi.mlp.0.weight": 3.321e-06, "net.8.layers.0.w.mlp.6.weight": 3.228e-06,
        "net.8.layers.1.u.linear.weight": 3.196e-06, "net.8.layers.0.phi.mlp.3.weight": 3.151e-06,
        "net.8.layers.0.w.mlp.0.bias": 3.100e-06, "net.8.layers.0.phi.mlp.6.weight": 3.020e-06,
        "net.8.layers.0.phi.mlp.1.bias": 2.998e-06, "net.8.layers.0.phi.mlp.0.bias": 2.988e-06,
        "net.8.layers.0.w.mlp.1.bias": 2.986e-06, "net.8.layers.0.phi.mlp.4.weight": 2.959e-06,
        "net.8.layers.0.w.mlp.3.bias": 2.905e-06, "net.8.layers.2.V.linear.weight": 2.854e-06,
        "net.8.layers.0.phi.mlp.3.bias": 2.799e-06, "net.3.embedding.weight": 2.786e-06, "net.8.layers.0.phi.mlp.6.bias": 2.762e-06,
        "net.8.layers.0.phi.mlp.4.bias": 2.742e-06, "net.8.layers.0.w.mlp.4.bias": 2.705e-06},
    2: {
        "net.7.layers.7.v.linear.weight": 5.089e-06, "net.3.embedding.weight": 4.926e-06, "net.7.layers.1.v.linear.weight": 4.727e-06,
        "net.7.layers.8.w.mlp.0.weight": 4.648e-06, "net.7.layers.0.w.mlp.0.weight": 4.619e-06,
        "net.7.layers.6.w.mlp.0.weight": 4.616e-06, "net.7.layers.9.v.linear.weight": 4.465e-06,
        "net.7.layers.5.v.linear.weight": 4.398e-06, "net.7.layers.4.w.mlp.0.weight": 4.092e-06,
        "net.7.layers.2.w.mlp.0.weight": 4.071e-06, "net.7.layers.3.v.linear.weight": 3.973e-06, "net.6.mlp.mlp.0.weight": 3.617e-06,
        "net.6.mlp.mlp.3.weight": 3.421e-06, "net.7.layers.0.phi.mlp.1.weight": 3.158e-06, "net.6.mlp.mlp.6.weight": 2.886e-06,
        "net.7.layers.0.phi.mlp.0.weight": 2.871e-06, "net.6.mlp.mlp.1.weight": 2.798e-06},
}


def halves(kind):
    return 2 if kind == "standard" else 1


def row_counts(c):
    """(node rows, vector rows, edge rows) of a call on case c"""
    R = halves(c["lk"]["kind"]) * c["B"]
    return R * c["A"], 3 * R * c["A"], R * int(c["model"]["src"].size)


def matrix_case(cell):
    variant, F, L, A, B, tpl, kind, gamma, a, center, rep, seed = cell
    return make_case(variant, F, L, A, B, tpl=tpl, kind=kind, gamma=gamma, a=a, center=center, seed=seed, repeat_ids=rep)
