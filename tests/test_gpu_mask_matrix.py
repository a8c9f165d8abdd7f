"""GPU: the masked twins of the three message kernels (per-molecule edge sets, include/ti_hip.h ti_painn_set_edge_mask) at every
template argument they are built for, against plain fp64 references.

painn_edge_mask_kernel<NBK, FIRST, LAST, PREC, WAVES, NS> (painn_edge_mask_nb{1,2,4,8}.hip): NBK = F / 16 for F in {32, 64, 128, 256};
(FIRST, LAST) = (true, true) only at L = 1, (false, false) only at L >= 3, the other two at every L >= 2 (L in {1, 3}, plus 5 at F = 256);
PREC 0 / 1 / 2 = f32 / f16x2 / the fp16 storage mode; NS follows the template's max_slots (painn_edge_kernel.hpp: launch_edge_nb), as
in test_gpu_f256.py: every molecule is masked on the complete directed graph of A atoms, so with 25 atoms every destination atom has 24
template rows and no 16-row block holds more than two destination atoms (NS = 2), with 7 atoms the runs are 6 rows long and blocks
hold up to four (NS = 4).  WAVES = 8 is the wide build, taken at >= 2048 molecule groups in f16x2 / f16 with at most two destination
atoms per block: 25 atoms, 2 * 2048 + 1 molecules, F in {32, 64, 128} (built, never launched: PREC 0, which keeps 4 waves).  painn_pair_mask_kernel<NBK, FIRST, LAST, PREC, WAVES> (painn_pair_mask_nb{1,2,4}.hip):
F in {32, 64, 128}, PREC 0 / 1, WAVES = 8 at >= 2048 groups in f16x2 (the same 25-atom batches).  painn_jvp_edge_mask_kernel<NBK, SPLIT> (painn_jvp_kernels.hip):
F in {32, 128, 256} here (F = 64 in test_gpu_edge_mask.py), f32 and f16x2.

Every masked batch is a per-molecule radius graph (cutoff at the 0.6 quantile of the pair distances) plus chain bonds over the
complete template; molecule 0's last atom sits far away and has no incoming edge.  Each molecule is compared with the fp64 oracle on
its OWN template (the present edges only).  Besides the matrices: the all-ones mask gives the unmasked bits at every width, depth,
precision and layout; the masked first-touch sums replace NaN-poisoned accumulators at full occupancy; the magnitude-edge fixtures of
test_gpu_parity.py / test_gpu_div_magnitudes.py stay exact under a mask (absent rows are evaluated and weighted by 0);
an absent atom 1e2 .. 1e6 away, not recentred, leaves the rest of its molecule as the oracle computes it.

Bars: DRIFT_TOL (1e-5 rel-L2) or 3x the fp32 oracle's own distance to fp64 where that is larger, per molecule; the fp16 storage mode
F16_TOL (1e-2); divergence DIV_ATOL * (|div| + 1), or max(DIV_REL * S, 3x the fp32 oracle's distance) with the case scale S of
test_gpu_div_magnitudes.py for the magnitude fixtures.  Every drift is re-run once and must be bit-identical.
Needs a real MI355X: `pytest -m gpu`.
"""
import functools
import types

import numpy as np
import pytest

from conftest import golden_weights, load_golden, pkg, rel_l2
from oracle import oracle
from test_gpu_div_magnitudes import CASES as DIV_CASES, DIV_REL
from test_gpu_divergence import DIV_ATOL
from test_gpu_f256 import F16_TOL
from test_gpu_parity import DRIFT_TOL, LNAFF_CASES, RANGE_CASES

pytestmark = pytest.mark.gpu

T = 0.37


# ------------------------------------------------------------------------------------------- masked problems
def presence(x, keep=0.6):
    """[B, A, A] bool, [b, s, d] = edge s -> d present in molecule b: radius graph at the `keep` quantile of the pair distances of
    molecules 1.. (so molecule 0's far atom does not move the cutoff) plus chain bonds 0 - 1 - ... - (A - 2), as test_gpu_edge_mask.case.
    Symmetric in (s, d)."""
    B, A, _ = x.shape
    off = ~np.eye(A, dtype=bool)
    dist = np.linalg.norm(x[:, :, None].astype(np.float64) - x[:, None, :], axis=-1)
    cutoff = float(np.quantile(dist[1:][:, off] if B > 1 else dist[:, off], keep))
    on = (dist <= cutoff) & off
    i = np.arange(A - 2)
    on[:, i, i + 1] = True
    on[:, i + 1, i] = True
    return on


def mask_words(on):
    """Bit s of mask[b, d] = on[b, s, d]."""
    A = on.shape[1]
    return (on.astype(np.uint64) << np.arange(A, dtype=np.uint64)[None, :, None]).sum(axis=1).astype(np.uint32)


def _weights(F, L, variant=0):
    ti = pkg()
    W = ti.weights
    return W.flatten_state_dict(ti.synthetic.painn_state_dict(variant, F, L, 25, seed=F + L), W.painn_param_spec(variant, F, L, 25))


@functools.lru_cache(maxsize=None)
def _problem(F, L, A, B, seed=0):
    """Complete template on A atoms, coordinates with molecule 0's last atom far away (no incoming edge), per-molecule presence."""
    ti = pkg()
    src, dst, et = ti.synthetic.fully_connected_template(A)
    x = ti.synthetic.molecule_coords(B, A, seed=seed + A)
    x[0, A - 1] += 25.0
    x = (x - x.mean(axis=1, keepdims=True)).astype(np.float32)
    on = presence(x)
    assert not on[0, :, A - 1].any()
    if B > 1:
        assert len({int(n) for n in on[1:].sum(axis=(1, 2))}) > 1 or B == 2       # the molecules really differ
    return types.SimpleNamespace(F=F, L=L, A=A, B=B, src=src, dst=dst, et=et, x=x, cond=ti.synthetic.ambient_cond(B, A), on=on,
                                 mask=mask_words(on), flat=_weights(F, L))


def engine(p, precision, layout=None, mask=True):
    ti = pkg()
    eng = ti.engine.PainnEngine(0, p.F, p.L, p.A, p.src, p.dst, p.et, np.arange(p.A), p.flat, temp_length=100.0, precision=precision)
    if layout is not None:
        eng.set_template(layout)
    if mask:
        eng.set_edge_mask(p.mask)
    return eng


def own_oracle(p, b):
    keep = p.on[b, p.src, p.dst]
    return oracle.PainnOracle(0, p.F, p.L, p.A, p.src[keep], p.dst[keep], p.et[keep], np.arange(p.A), p.flat, temp_length=100.0)


@functools.lru_cache(maxsize=None)
def _oracle_drift(F, L, A, B, idx=None):
    """Per molecule (index idx, default all): (fp64 drift on its own graph, fp32 oracle's distance to it)."""
    p = _problem(F, L, A, B)
    out = []
    for b in (range(B) if idx is None else idx):
        orc = own_oracle(p, b)
        xb, cb = p.x[b:b + 1], p.cond[b:b + 1]
        ref = orc.drift(xb, T, cb, precision=64)
        out.append((ref, rel_l2(orc.drift(xb, T, cb), ref)))
    return out


def check_drift(got, refs, precision, idx=None):
    assert np.isfinite(got).all()
    for k, (ref, floor) in enumerate(refs):
        b = k if idx is None else idx[k]
        bar = F16_TOL if precision == "f16" else max(DRIFT_TOL, 3 * floor)
        err = rel_l2(got[b:b + 1], ref)
        assert err < bar, (b, err, bar)


NS_CASES = pytest.mark.parametrize("A,B", [(25, 3), (7, 5)], ids=["NS2", "NS4"])


# ------------------------------------------------------------------------------------------- 1. directed instantiation matrix
@NS_CASES
@pytest.mark.parametrize("template", ["throughput", "latency"])
@pytest.mark.parametrize("precision", ["f32", "f16x2", "f16"])
@pytest.mark.parametrize("F,L", [(F, L) for F in (32, 64, 128, 256) for L in (1, 3)] + [(256, 5)])
def test_masked_directed_instantiations_vs_fp64_oracle(F, L, precision, template, A, B):
    p = _problem(F, L, A, B)
    eng = engine(p, precision, template)
    assert eng.template_for(B) == template                  # a pinned layout that exists for this molecule, not a fall-back
    got = eng.drift(p.x, T, p.cond)
    check_drift(got, _oracle_drift(F, L, A, B), precision)
    np.testing.assert_array_equal(eng.drift(p.x, T, p.cond), got)
    eng.close()


# ------------------------------------------------------------------------------------------- 2. pair instantiation matrix
@NS_CASES
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("F", [32, 64, 128])
def test_masked_pair_instantiations_vs_fp64_oracle(F, L, precision, A, B):
    p = _problem(F, L, A, B)
    eng = engine(p, precision, "pair")
    assert eng.template_for(B) == "pair"                    # radius + bond graphs: symmetric sets
    got = eng.drift(p.x, T, p.cond)
    check_drift(got, _oracle_drift(F, L, A, B), precision)
    np.testing.assert_array_equal(eng.drift(p.x, T, p.cond), got)
    eng.close()


# ------------------------------------------------------------------------------------------- 3. 8-wave masked builds
# The wide directed build is instantiated for NS = 2 only (launch_edge_nb: max_slots <= 2), so it needs destination runs of more than
# 8 rows: 25 atoms (24 rows each) at G = 2 molecules per throughput group, 2 * 2048 + 1 molecules = 2049 groups.  (6 atoms give 5-row
# runs, up to four destination atoms per block: the 4-wave NS = 4 build at any batch size.)
WIDE_A, WIDE_B = 25, 2 * 2048 + 1
WIDE_IDX = tuple(range(40)) + tuple(range(WIDE_B - 40, WIDE_B))


@pytest.mark.parametrize("layout,precision", [("throughput", "f16x2"), ("throughput", "f16"), ("pair", "f16x2")])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("F", [32, 64, 128])
def test_masked_wide_workgroups(F, L, layout, precision):
    p = _problem(F, L, WIDE_A, WIDE_B)
    assert len(np.unique(p.mask, axis=0)) > 1000             # a mask that differs from molecule to molecule
    eng = engine(p, precision, layout)
    assert eng.template_for(WIDE_B) == layout
    got = eng.drift(p.x, T, p.cond)
    check_drift(got, _oracle_drift(F, L, WIDE_A, WIDE_B, WIDE_IDX), precision, WIDE_IDX)
    np.testing.assert_array_equal(eng.drift(p.x, T, p.cond), got)
    # the same molecules under the same mask rows through the narrow build (a batch below the threshold): bit for bit
    eng.set_edge_mask(p.mask[:800])
    np.testing.assert_array_equal(eng.drift(p.x[:800], T, p.cond[:800]), got[:800])
    eng.close()


# ------------------------------------------------------------------------------------------- 4. all-ones mask = no mask
def _layouts(F, precision):
    return ["throughput", "latency"] + (["pair"] if F <= 128 and precision != "f16" else [])


@pytest.mark.parametrize("precision", ["f32", "f16x2", "f16"])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("F", [32, 64, 128, 256])
def test_all_ones_mask_equals_no_mask_bit_for_bit_at_every_width(F, L, precision):
    p = _problem(F, L, 7, 5)
    ones = np.full((p.B, p.A), (1 << p.A) - 1, np.uint32)
    for layout in _layouts(F, precision):
        res = []
        for m in (None, ones):
            eng = engine(p, precision, layout, mask=False)
            eng.set_edge_mask(m)
            assert eng.template_for(p.B) == layout
            r = [eng.drift(p.x, T, p.cond)]
            if precision != "f16":                           # the fp16 storage mode has no tangent path
                r += list(eng.drift_div(p.x, T, p.cond))
                r += list(eng.drift_div_est(p.x, T, p.cond, n_probes=3, probe_seed=5))
            res.append(r)
            eng.close()
        assert np.isfinite(res[0][0]).all()
        for a, b in zip(*res):
            np.testing.assert_array_equal(a, b, err_msg=layout)


# ------------------------------------------------------------------------------------------- 5. masked tangent kernels
TAN_L, TAN_A, TAN_B = 2, 7, 4


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("F", [32, 128, 256])
def test_masked_tangent_kernels_per_molecule(F, precision):
    ti = pkg()
    p = _problem(F, TAN_L, TAN_A, TAN_B)
    eng = engine(p, precision)
    xdot = np.random.RandomState(7).standard_normal(p.x.shape).astype(np.float32)
    out, div = eng.drift_div(p.x, T, p.cond)
    b, tan = eng.jvp(p.x, xdot, T, p.cond)
    grid = ti.engine.time_grid(0.0, 1.0, 4)
    path, dl, _ = eng.rollout_dlogp(p.x, p.cond, grid, scheme="heun")
    assert np.isfinite(div).all() and np.isfinite(tan).all() and np.isfinite(dl).all()
    for m in range(p.B):
        orc, xm, xd, cm = own_oracle(p, m), p.x[m:m + 1], xdot[m:m + 1], p.cond[m:m + 1]
        ro, rd = orc.drift_div(xm, T, cm, precision=64)
        assert rel_l2(out[m:m + 1], ro) < DRIFT_TOL, m
        assert abs(div[m] - rd[0]) < DIV_ATOL * (abs(rd[0]) + 1.0), (m, div[m], rd[0])
        rb, rt = orc.jvp(xm, xd, T, cm, precision=64)
        floor = rel_l2(orc.jvp(xm, xd, T, cm, precision=32)[1], rt)
        assert rel_l2(b[m:m + 1], rb) < DRIFT_TOL, m
        assert rel_l2(tan[m:m + 1], rt) < max(DRIFT_TOL, 3 * floor), (m, rel_l2(tan[m:m + 1], rt), floor)
        rp, rdl, _ = orc.rollout_dlogp(xm, cm, grid, scheme="heun", precision=64)
        assert rel_l2(path[:, m:m + 1] - path[0, m:m + 1], rp - rp[0]) < 1e-4, m
        assert np.abs(dl[:, m] - rdl[:, 0]).max() < 1e-4 * (np.abs(rdl).max() + 1.0), m
    eng.close()


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_f256_hutchinson_molecule_in_a_masked_batch_equals_it_alone(precision):
    ti = pkg()
    p = _problem(256, TAN_L, TAN_A, TAN_B)
    eng = engine(p, precision)
    out, est = eng.drift_div_est(p.x, 0.6, p.cond, n_probes=4, probe_seed=9, traj_offset=100)
    for m in range(p.B):
        keep = p.on[m, p.src, p.dst]
        alone = ti.engine.PainnEngine(0, p.F, p.L, p.A, p.src[keep], p.dst[keep], p.et[keep], np.arange(p.A), p.flat, temp_length=100.0,
                                      precision=precision)
        o1, e1 = alone.drift_div_est(p.x[m:m + 1], 0.6, p.cond[m:m + 1], n_probes=4, probe_seed=9, traj_offset=100 + m)
        assert rel_l2(out[m:m + 1], o1) < 3e-6, m
        assert abs(est[m] - e1[0]) < 1e-5 * (abs(e1[0]) + 1.0), (m, est[m], e1[0])
        alone.close()
    eng.close()


# ------------------------------------------------------------------------------------------- 6. first touch at full occupancy, F = 256
OCC_B = 8192                                                 # one resident workgroup per CU at F = 256: >= 1024 workgroups per launch


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("template", ["throughput", "latency"])
def test_f256_masked_first_touch_full_occupancy(template, precision, monkeypatch):
    """NaN-poisoned accumulators before every evaluation: the masked first-touch path returns exactly what the zeroing path
    (TI_ZERO_ACC=1: memsets, adds only) returns, molecule 0's atom without incoming edges included."""
    p = _problem(256, 5, 25, OCC_B)

    def make(zeroing):
        if zeroing:
            monkeypatch.setenv("TI_ZERO_ACC", "1")
        eng = engine(p, precision, template)
        monkeypatch.delenv("TI_ZERO_ACC", raising=False)
        assert eng.template_for(OCC_B) == template
        return eng

    eng = make(True)
    ref = eng.drift(p.x, 0.5, p.cond)
    eng.close()
    assert np.isfinite(ref).all()
    eng = make(False)
    for _ in range(2):                                       # the second call meets the first one's leftovers as well
        eng.debug_poison(OCC_B, float("nan"))
        np.testing.assert_array_equal(eng.drift(p.x, 0.5, p.cond), ref)
    eng.close()


# ------------------------------------------------------------------------------------------- 7. magnitude edges under a mask
def golden_mask(g):
    """Symmetric presence over the fixture's template: molecule b loses the pair (b, b + 1); molecule 0 also loses every edge of its
    last atom."""
    A, B = int(g["A"]), int(g["B"])
    src, dst = g["edge_src"].astype(np.int64), g["edge_dst"].astype(np.int64)
    on = np.zeros((B, A, A), bool)
    on[:, src, dst] = True
    for b in range(B):
        on[b, b, b + 1] = on[b, b + 1, b] = False
    on[0, A - 1, :] = on[0, :, A - 1] = False
    return on


def golden_engine(g, precision, on):
    ti = pkg()
    eng = ti.engine.PainnEngine(int(g["variant"]), int(g["F"]), int(g["L"]), int(g["A"]), g["edge_src"], g["edge_dst"], g["edge_type"],
                                g["atom_ids"], golden_weights(g), temp_length=float(g["temp_length"]), temperatures=g["temperatures"],
                                precision=precision)
    eng.set_edge_mask(mask_words(on))
    return eng


def golden_own_oracle(g, on, b):
    keep = on[b, g["edge_src"].astype(np.int64), g["edge_dst"].astype(np.int64)]
    return oracle.PainnOracle(int(g["variant"]), int(g["F"]), int(g["L"]), int(g["A"]), g["edge_src"][keep], g["edge_dst"][keep],
                              g["edge_type"][keep], g["atom_ids"], golden_weights(g), temp_length=float(g["temp_length"]),
                              temperatures=g["temperatures"])


@functools.lru_cache(maxsize=None)
def _golden_oracle_drift(name):
    """[(t, [(fp64 drift, fp32 distance) per molecule])] of a fixture under golden_mask."""
    g = load_golden(name)
    on = golden_mask(g)
    res = []
    for t in g["ts"]:
        per = []
        for b in range(int(g["B"])):
            orc, xb, cb = golden_own_oracle(g, on, b), g["x"][b:b + 1], g["cond"][b:b + 1]
            ref = orc.drift(xb, float(t), cb, precision=64)
            per.append((ref, rel_l2(orc.drift(xb, float(t), cb), ref)))
        res.append((float(t), per))
    return res


def _golden_layouts(names):
    """(name, layout): throughput for every fixture, pair where a pair layout exists (F <= 128)."""
    return [(n, t) for n in names for t in ("throughput", "pair") if t == "throughput" or int(load_golden(n)["F"]) <= 128]


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("name,template", _golden_layouts(RANGE_CASES + LNAFF_CASES))
def test_masked_magnitude_edges_vs_fp64_oracle(name, template, precision):
    """Un-normalised streams at 1e3 .. 1e6 or 1e-7 .. 1e-9, an edge of length 1e-4, LayerNorm affines at 1e-5 .. 1e3: absent rows
    are still evaluated at these magnitudes and must leave the present atoms' sums exactly as the oracle on the remaining graph has them."""
    g = load_golden(name)
    on = golden_mask(g)
    eng = golden_engine(g, precision, on)
    eng.set_template(template)
    assert eng.template_for(int(g["B"])) == template
    for t, per in _golden_oracle_drift(name):
        got = eng.drift(g["x"], t, g["cond"])
        assert np.isfinite(got).all(), (name, t)
        for b, (ref, floor) in enumerate(per):
            err = rel_l2(got[b:b + 1], ref)
            assert err < max(DRIFT_TOL, 3 * floor), (name, t, b, err, floor)
        np.testing.assert_array_equal(eng.drift(g["x"], t, g["cond"]), got)
    eng.close()


@functools.lru_cache(maxsize=None)
def _golden_oracle_div(name):
    """Per molecule under golden_mask: (div64, |div32 - div64|, S = sum_i |d b_i / d x_i| from the fp64 oracle's unit-seed JVPs)."""
    g = load_golden(name)
    on = golden_mask(g)
    A, t = int(g["A"]), float(g["t"])
    out = []
    for b in range(int(g["B"])):
        orc, xb, cb = golden_own_oracle(g, on, b), g["x"][b:b + 1], g["cond"][b:b + 1]
        d64 = float(orc.drift_div(xb, t, cb, precision=64)[1][0])
        d32 = float(orc.drift_div(xb, t, cb, precision=32)[1][0])
        S = 0.0
        for i in range(3 * A):
            e = np.zeros((1, A, 3), np.float32)
            e.reshape(-1)[i] = 1.0
            S += abs(float(orc.jvp(xb, e, t, cb, precision=64)[1].reshape(-1)[i]))
        out.append((d64, abs(d32 - d64), S))
    return out


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("name", DIV_CASES)
def test_masked_divergence_magnitude_edges_vs_fp64_oracle(name, precision):
    g = load_golden(name)
    on = golden_mask(g)
    eng = golden_engine(g, precision, on)
    eng.set_template("throughput")
    t = float(g["t"])
    b, div = eng.drift_div(g["x"], t, g["cond"])
    assert np.isfinite(b).all() and np.isfinite(div).all(), (name, div)
    for m, (d64, floor, S) in enumerate(_golden_oracle_div(name)):
        bar = max(DIV_REL * S, 3.0 * floor)
        assert bar < 0.1 * S, (name, m, bar, S)              # not vacuous
        assert abs(div[m] - d64) < bar, (name, m, div[m], d64, bar)
    np.testing.assert_array_equal(eng.drift_div(g["x"], t, g["cond"])[1], div)
    eng.close()


# ------------------------------------------------------------------------------------------- 8. far absent atoms
@functools.lru_cache(maxsize=None)
def _far_problem(F, dist):
    """7 atoms, 3 molecules, not recentred: molecule 0's last atom and molecule 1's atom 2 moved `dist` away, every edge to and from
    them masked; molecule 2 keeps the complete graph."""
    p = _problem(F, 3, 7, 3)
    x = p.x.copy()
    x[0, 6] += np.float32([dist, 0.0, 0.0])
    x[1, 2] += np.float32([0.0, -dist, 0.5 * dist])
    on = np.broadcast_to(~np.eye(7, dtype=bool), (3, 7, 7)).copy()
    for b, a in ((0, 6), (1, 2)):
        on[b, a, :] = on[b, :, a] = False
    q = types.SimpleNamespace(**{**vars(p), "x": x.astype(np.float32), "on": on, "mask": mask_words(on)})
    refs = []
    for b in range(3):
        orc, xb, cb = own_oracle(q, b), q.x[b:b + 1], q.cond[b:b + 1]
        ref = orc.drift(xb, T, cb, precision=64)
        refs.append((ref, rel_l2(orc.drift(xb, T, cb), ref)))
    return q, refs


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("F,layout", [(128, "throughput"), (128, "latency"), (128, "pair"), (256, "throughput"), (256, "latency")])
@pytest.mark.parametrize("dist", [1e2, 1e4, 1e6])
def test_far_absent_atoms_leave_the_rest_exact(dist, F, layout, precision):
    q, refs = _far_problem(F, dist)
    eng = engine(q, precision, layout)
    assert eng.template_for(q.B) == layout
    got = eng.drift(q.x, T, q.cond)
    check_drift(got, refs, precision)
    np.testing.assert_array_equal(eng.drift(q.x, T, q.cond), got)
    eng.close()
