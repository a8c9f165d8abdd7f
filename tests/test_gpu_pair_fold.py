"""The pair-major message kernel with the cross term folded into dv (csrc/painn_pair_kernel_body.inc, FOLD; ti_internal.hpp
pair_folds_cross): on the split path each (row block, slot) crosses its sum of cg * dir with v[dst] in registers, adds it to the dv sums
and never writes cacc; the update kernel after it (painn_update_kernel<.., FOLDED>) neither reads cacc nor crosses it.  Both builds
fold: the 4-wave one below 2048 molecule groups, the 8-wave one from there on (4 molecules per group at A = 18: 8192 molecules).
These tests pin that nothing reads the stale cacc of a folded launch, that the directed launches after one (the divergence) are
unaffected, and that the pair and directed layouts still agree, with and without an edge mask, in both builds.
Needs a real MI355X: `pytest -m gpu`.
"""
import numpy as np
import pytest

from conftest import pkg, rel_l2
from oracle import oracle
from test_gpu_edge_mask import case, engine
from test_gpu_parity import DRIFT_TOL

pytestmark = pytest.mark.gpu

F, L, A = 128, 5, 18
WIDE_B = 8192 + 4                            # > 2048 groups of 4 molecules: the 8-wave build


def headline_model():
    ti = pkg()
    syn, W = ti.synthetic, ti.weights
    src, dst, et = syn.fully_connected_template(A)
    flat = W.flatten_state_dict(syn.painn_state_dict(0, F, L, 25, seed=0), W.painn_param_spec(0, F, L, 25))
    return src, dst, et, flat


def headline_engine(precision, layout):
    src, dst, et, flat = headline_model()
    eng = pkg().engine.PainnEngine(0, F, L, A, src, dst, et, np.arange(A), flat, temp_length=100.0, precision=precision)
    eng.set_template(layout)
    return eng


def inputs(B, seed=0):
    syn = pkg().synthetic
    return syn.molecule_coords(B, A, seed=seed), syn.ambient_cond(B, A)


@pytest.mark.parametrize("B", [1000, WIDE_B])
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_pair_drift_ignores_poisoned_cross_accumulator(precision, B):
    """cacc filled with NaN before the call (debug_poison fills dsacc / dvacc / cacc; the first-touch launches replace the first two):
    the drift is bit for bit the drift with all three zeroed.  For f16x2 this shows that no folded launch and no folded update reads
    cacc; for f32 (cacc still in use) that its first-touch writes replace it."""
    eng = headline_engine(precision, "pair")
    assert eng.template_for(B) == "pair"
    x, cond = inputs(B)
    eng.debug_poison(B, 0.0)
    ref = eng.drift(x, 0.5, cond)
    assert np.isfinite(ref).all()
    for _ in range(2):
        eng.debug_poison(B, float("nan"))
        np.testing.assert_array_equal(eng.drift(x, 0.5, cond), ref)
    eng.close()


def test_divergence_after_a_folded_pair_drift_equals_a_fresh_handle():
    """The exact divergence walks directed rows and reads the primal cacc of its own launches: a pair drift on the same handle before it
    (which leaves cacc as it was) changes nothing, bit for bit."""
    B = 8
    x, cond = inputs(B, seed=3)
    fresh = headline_engine("f16x2", "pair")
    d0, div0 = fresh.drift_div(x, 0.5, cond)
    fresh.close()
    eng = headline_engine("f16x2", "pair")
    big_x, big_cond = inputs(WIDE_B, seed=4)
    eng.debug_poison(WIDE_B, float("nan"))
    assert np.isfinite(eng.drift(big_x, 0.5, big_cond)).all()
    eng.drift(x, 0.5, cond)
    d1, div1 = eng.drift_div(x, 0.5, cond)
    np.testing.assert_array_equal(div1, div0)
    np.testing.assert_array_equal(d1, d0)
    eng.close()


@pytest.mark.parametrize("B", [64, WIDE_B])
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_pair_and_directed_layouts_agree(precision, B):
    x, cond = inputs(B, seed=1)
    out = {}
    for layout in ("pair", "throughput"):
        eng = headline_engine(precision, layout)
        assert eng.template_for(B) == layout
        out[layout] = eng.drift(x, 0.5, cond)
        eng.close()
    assert np.isfinite(out["pair"]).all()
    assert rel_l2(out["pair"], out["throughput"]) < DRIFT_TOL
    src, dst, et, flat = headline_model()
    orc = oracle.PainnOracle(0, F, L, A, src, dst, et, np.arange(A), flat, temp_length=100.0)
    idx = np.r_[0:3, B - 3:B]
    assert rel_l2(out["pair"][idx], orc.drift(x[idx], 0.5, cond[idx], precision=64)) < DRIFT_TOL


@pytest.mark.parametrize("reps", [1, 745])
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
def test_masked_pair_and_directed_layouts_agree(precision, reps):
    """Per-molecule radius graphs (one atom without incoming edges); 745 copies of the 11 molecules make 8195: the 8-wave build."""
    c = case(18, 11, variant=0, F=128, L=4)
    x, cond, mask = (np.ascontiguousarray(np.tile(a, (reps,) + (1,) * (a.ndim - 1))) for a in (c.x, c.cond, c.mask))
    B = x.shape[0]
    out = {}
    for layout in ("pair", "throughput"):
        eng = engine(c, precision)
        eng.set_template(layout)
        eng.set_edge_mask(mask)
        assert eng.template_for(B) == layout
        out[layout] = eng.drift(x, 0.4, cond)
        eng.close()
    assert np.isfinite(out["pair"]).all()
    err = np.linalg.norm((out["pair"] - out["throughput"]).reshape(B, -1), axis=1) / np.linalg.norm(out["throughput"].reshape(B, -1), axis=1)
    assert err.max() < 3e-5, (int(err.argmax()), float(err.max()))       # per molecule, as test_gpu_pair.py bounds it
    for b in range(c.B):                                     # the first copy against each molecule's own graph on the CPU oracle
        s, d, t = c.tpls[b]
        ref = oracle.PainnOracle(0, c.F, c.L, c.A, s, d, t, np.arange(c.A), c.flat, temp_length=c.temp_length).drift(
            c.x[b:b + 1], 0.4, c.cond[b:b + 1], precision=64)
        assert rel_l2(out["pair"][b:b + 1], ref) < DRIFT_TOL, b
