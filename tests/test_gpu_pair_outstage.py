"""The output stage of the pair-major message kernel (csrc/painn_pair_kernel_body.inc): the bias of an output slice seeds its
accumulators, rows of pairs that do not exist move no e row, no parked encoding and no edge_dir, and the node arrays are addressed from
the group's base.  Pinned here at the shapes where those paths differ: F = 32 and 128 (one and four 32-feature slices), 3, 5 and 18
atoms (blocks of mostly absent rows and empty slots; the headline template), 1, 6 and 9 molecules (ragged last group), 1, 2 and 3
layers (first and last layer in one launch; first then last; a middle layer), both matrix paths, and the masked twin with one pair
removed per molecule.  Bars: those of tests/test_gpu_pair.py (DRIFT_TOL on the drift and on s / v / e after every layer, against the
fp64 oracle).  Needs a real MI355X: `pytest -m gpu`.
"""
import functools

import numpy as np
import pytest

from conftest import pkg, rel_l2
from oracle import oracle
from test_gpu_parity import DRIFT_TOL

pytestmark = pytest.mark.gpu

BATCHES = (9, 6, 1)
T = 0.4


@functools.lru_cache(maxsize=None)
def model(F, L, A):
    ti = pkg()
    syn, W = ti.synthetic, ti.weights
    src, dst, et = syn.fully_connected_template(A)
    flat = W.flatten_state_dict(syn.painn_state_dict(0, F, L, 25, seed=F + A), W.painn_param_spec(0, F, L, 25))
    x, cond = syn.molecule_coords(max(BATCHES), A, seed=A), syn.ambient_cond(max(BATCHES), A)
    for a in (src, dst, et, flat, x, cond):
        a.setflags(write=False)
    return src, dst, et, flat, x, cond


def pair_engine(F, L, A, precision):
    ti = pkg()
    src, dst, et, flat, _, _ = model(F, L, A)
    eng = ti.engine.PainnEngine(0, F, L, A, src, dst, et, np.arange(A), flat, temp_length=100.0, precision=precision)
    _lib = ti._lib
    _lib.check(_lib.lib().ti_painn_set_template(eng.h, eng.TEMPLATES["pair"]))       # TI_TEMPLATE_PAIR
    return eng


def make_oracle(F, L, A, src, dst, et):
    return oracle.PainnOracle(0, F, L, A, src, dst, et, np.arange(A), model(F, L, A)[3], temp_length=100.0)


def removed_pair(b, A):
    i = b % A
    return i, (i + 1 + (b // A) % (A - 1)) % A


def pair_mask(B, A):
    """All template edges but one pair per molecule, both directions: bit s of mask[b, d] = edge s -> d exists."""
    m = np.zeros((B, A), np.uint32)
    for b in range(B):
        i, j = removed_pair(b, A)
        for d in range(A):
            for s in range(A):
                if s != d and {s, d} != {i, j}:
                    m[b, d] |= np.uint32(1 << s)
    return m


def stages(L):
    return [s for l in range(L) for s in ((1 + 2 * l, f"msg{l}"), (2 + 2 * l, f"upd{l}"))]


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("A", [3, 5, 18])
@pytest.mark.parametrize("F", [32, 128])
def test_drift_and_taps_against_the_fp64_oracle(F, A, L, precision):
    src, dst, et, _, x9, cond9 = model(F, L, A)
    eng, orc = pair_engine(F, L, A, precision), make_oracle(F, L, A, src, dst, et)
    try:
        for B in BATCHES:
            x, cond = x9[:B], cond9[:B]
            assert eng.template_for(B) == "pair"
            got = eng.drift(x, T, cond)
            err = rel_l2(got, orc.drift(x, T, cond, precision=64))
            print(f"F {F} A {A} L {L} {precision} B {B}: drift rel-L2 {err:.2e}")
            assert np.isfinite(got).all() and err < DRIFT_TOL, (B, err)
            for stage, tag in stages(L):
                eng.debug_tap(stage)
                eng.drift(x, T, cond)
                _, taps = orc.drift(x, T, cond, precision=64, tap_stage=stage)
                s, v = eng.debug_read("s", B), eng.debug_read("v", B).transpose(0, 1, 3, 2)
                assert rel_l2(s, taps["s"]) < DRIFT_TOL, (B, tag, "s")
                assert rel_l2(v, taps["v"]) < DRIFT_TOL, (B, tag, "v")
                if tag.startswith("msg") and int(tag[3:]) < L - 1:
                    assert rel_l2(eng.debug_read("e", B), taps["e"]) < DRIFT_TOL, (B, tag, "e")
            eng.debug_tap(-1)
    finally:
        eng.debug_tap(-1)
        eng.close()


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("A", [3, 5, 18])
@pytest.mark.parametrize("F", [32, 128])
def test_masked_twin_one_pair_removed_per_molecule(F, A, L, precision):
    """Every molecule misses another pair: drift and s / v / e of the edges it keeps, per molecule against the oracle of its own graph."""
    src, dst, et, _, x9, cond9 = model(F, L, A)
    eng = pair_engine(F, L, A, precision)
    try:
        for B in BATCHES:
            x, cond = x9[:B], cond9[:B]
            eng.set_edge_mask(pair_mask(B, A))
            assert eng.template_for(B) == "pair"
            got = eng.drift(x, T, cond)
            assert np.isfinite(got).all()
            np.testing.assert_array_equal(eng.drift(x, T, cond), got)
            taps = {}
            for stage, tag in stages(L):
                eng.debug_tap(stage)
                eng.drift(x, T, cond)
                taps[tag] = (eng.debug_read("s", B), eng.debug_read("v", B).transpose(0, 1, 3, 2),
                             eng.debug_read("e", B) if tag.startswith("msg") and int(tag[3:]) < L - 1 else None)
            eng.debug_tap(-1)
            for b in range(B):
                i, j = removed_pair(b, A)
                keep = np.array([{int(s), int(d)} != {i, j} for s, d in zip(src, dst)])
                orc = make_oracle(F, L, A, src[keep], dst[keep], et[keep])
                xb, cb = x[b:b + 1], cond[b:b + 1]
                assert rel_l2(got[b:b + 1], orc.drift(xb, T, cb, precision=64)) < DRIFT_TOL, (B, b)
                for stage, tag in stages(L):
                    _, ref = orc.drift(xb, T, cb, precision=64, tap_stage=stage)
                    s, v, e = taps[tag]
                    assert rel_l2(s[b:b + 1], ref["s"]) < DRIFT_TOL, (B, b, tag, "s")
                    assert rel_l2(v[b:b + 1], ref["v"]) < DRIFT_TOL, (B, b, tag, "v")
                    if e is not None:
                        assert rel_l2(e[b:b + 1][:, keep], ref["e"]) < DRIFT_TOL, (B, b, tag, "e")
            eng.set_edge_mask(None)
    finally:
        eng.debug_tap(-1)
        eng.close()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("F,A,L", [(32, 3, 3), (32, 18, 2), (128, 5, 3), (128, 18, 3), (128, 18, 1)])
def test_reruns_slices_and_stale_workspace_are_bit_identical(F, A, L, precision, masked):
    """Two runs agree bit for bit; the first eight molecules (whole groups: a group holds 1, 2, 4 or 8) evaluated alone equal the same
    molecules inside the batch of nine; with the edge state, the parked encoding and edge_dir and the per-atom accumulators filled with
    NaN, then with 1e30, before the call (debug_poison), the result does not move: rows of absent pairs are neither read nor needed, and
    every other row is written before it is read."""
    _, _, _, _, x, cond = model(F, L, A)
    B = max(BATCHES)
    eng = pair_engine(F, L, A, precision)
    try:
        mask = pair_mask(B, A) if masked else None
        if masked:
            eng.set_edge_mask(mask)
        assert eng.template_for(B) == "pair"
        ref = eng.drift(x, T, cond)
        assert np.isfinite(ref).all()
        np.testing.assert_array_equal(eng.drift(x, T, cond), ref)
        for poison in (float("nan"), 1e30):
            eng.debug_poison(B, poison)
            np.testing.assert_array_equal(eng.drift(x, T, cond), ref)
            eng.debug_poison(B, poison)
            eng.debug_tap(2 * L - 1)                               # the last message layer: its sums before the update consumes them
            eng.drift(x, T, cond)
            assert np.isfinite(eng.debug_read("s", B)).all() and np.isfinite(eng.debug_read("v", B)).all()
            eng.debug_tap(-1)
        if masked:
            eng.set_edge_mask(mask[:8])
        eng.debug_poison(B, float("nan"))
        np.testing.assert_array_equal(eng.drift(x[:8], T, cond[:8]), ref[:8])
    finally:
        eng.debug_tap(-1)
        eng.close()
