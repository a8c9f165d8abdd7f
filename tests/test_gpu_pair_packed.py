"""The packed pair-major template on the GPU (csrc/pair_template.hpp: build_pair_template_packed; the GENERAL builds of
csrc/painn_pair_kernel.hpp): a group's leading row blocks are 4 x 4 tiles, walked by the tile launch; the rest hold 16 unrelated pairs
each, walked by a second launch whose rows add their two contributions to their own two atoms.  Shapes: A = 18 is the smallest
complete graph with full tiles and general blocks at 4 molecules per group (36 + 3 blocks); A = 12 takes groups of 8 molecules with
9 general blocks in 33 (the generic pass alone); A = 9 is kept as a case although the builder, which weighs a general block at its
measured cost, leaves it on tiles (an unweighted pass put it on 16 + 5 blocks and lost 10 % of its steps/s: DESIGN.md 4.0b); B = 6
and 9 leave a ragged last group; A = 3 and 5 have no atom eligible for a general row and must reproduce the
tile-only template (TI_PAIR_PACKED=0 when the handle is created) bit for bit.  General blocks exist on the split path (f16x2); f32
handles keep the tile-only template (ti_internal.hpp: pair_general_build_exists) and are held to the same bars on it.
Bars: DRIFT_TOL of tests/test_gpu_parity.py against the fp64 oracle, on the drift and on s / v / e after every stage.
Needs a real MI355X: `pytest -m gpu`.
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
WIDE_B = 8194                                # 2049 groups of 4 molecules at A = 18: the 8-wave builds, ragged last group


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


def pair_engine(monkeypatch, F, L, A, precision="f16x2", packed=True, table=True, layout="pair"):
    """A handle with `layout` pinned.  packed = False: created with TI_PAIR_PACKED=0 (tile blocks only); table = False: with
    TI_PHI0_TABLE=0 (layer 0 computes its phi branch)."""
    ti = pkg()
    src, dst, et, flat = model(F, L, A)[:4]
    monkeypatch.delenv("TI_TEMPLATE", raising=False)
    for name, on in (("TI_PAIR_PACKED", packed), ("TI_PHI0_TABLE", table)):
        if on:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, "0")
    eng = ti.engine.PainnEngine(0, F, L, A, src, dst, et, np.arange(A), flat, temp_length=100.0, precision=precision)
    monkeypatch.delenv("TI_PAIR_PACKED", raising=False)
    monkeypatch.delenv("TI_PHI0_TABLE", raising=False)
    eng.set_template(layout)
    return eng


def has_general(eng):
    G, nblk, n_tile = eng.debug_pair_blocks()
    return n_tile < nblk


def make_oracle(F, L, A, src, dst, et):
    return oracle.PainnOracle(0, F, L, A, src, dst, et, np.arange(A), model(F, L, A)[3], temp_length=100.0)


def stages(L):
    return [s for l in range(L) for s in ((1 + 2 * l, f"msg{l}"), (2 + 2 * l, f"upd{l}"))]


def removed_pair(b, A):
    """molecule b loses the pair (b, b + 1): at A = 18 a twin pair (2a, 2a + 1) for even b -- a general row of the packed template --
    and a pair of two different twins for odd b -- a tile row"""
    return b % A, (b + 1) % A


def pair_mask(B, A):
    m = np.zeros((B, A), np.uint32)
    for b in range(B):
        i, j = removed_pair(b, A)
        for d in range(A):
            for s in range(A):
                if s != d and {s, d} != {i, j}:
                    m[b, d] |= np.uint32(1 << s)
    return m


def test_template_of_the_headline_molecule(monkeypatch):
    eng = pair_engine(monkeypatch, 32, 1, 18)
    old = pair_engine(monkeypatch, 32, 1, 18, packed=False)
    f32 = pair_engine(monkeypatch, 32, 1, 18, precision="f32")
    a12 = pair_engine(monkeypatch, 32, 1, 12)
    try:
        assert eng.debug_pair_blocks() == (4, 39, 36) and old.debug_pair_blocks() == (4, 45, 45) and f32.debug_pair_blocks() == (4, 45, 45)
        assert a12.debug_pair_blocks() == (8, 33, 24)
    finally:
        eng.close(); old.close(); f32.close(); a12.close()


@pytest.mark.parametrize("precision", ["f32", "f16x2"])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("A", [9, 12, 18])
@pytest.mark.parametrize("F", [32, 128])
def test_drift_and_taps_against_the_fp64_oracle(monkeypatch, F, A, L, precision):
    src, dst, et, _, x9, cond9 = model(F, L, A)
    eng, orc = pair_engine(monkeypatch, F, L, A, precision), make_oracle(F, L, A, src, dst, et)
    try:
        assert has_general(eng) == (precision == "f16x2" and A != 9)         # general blocks are in use wherever their builds exist and pay
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


@pytest.mark.parametrize("A", [3, 5])
def test_molecules_without_eligible_atoms_keep_the_tile_template_bit_for_bit(monkeypatch, A):
    F, L, B = 32, 3, 9
    _, _, _, _, x, cond = model(F, L, A)
    eng, old = pair_engine(monkeypatch, F, L, A), pair_engine(monkeypatch, F, L, A, packed=False)
    try:
        assert not has_general(eng) and eng.debug_pair_blocks() == old.debug_pair_blocks()
        ref = old.drift(x, T, cond)
        assert np.isfinite(ref).all()
        np.testing.assert_array_equal(eng.drift(x, T, cond), ref)
    finally:
        eng.close(); old.close()


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("F", [32, 128])
def test_masked_twin_one_pair_removed_per_molecule(monkeypatch, F, L):
    """A = 18, B = 9: even molecules lose a pair that sits in a general row, odd ones a pair in a tile row; drift and s / v / e of the
    edges a molecule keeps, per molecule against the oracle of its own graph."""
    A, B = 18, 9
    src, dst, et, _, x, cond = model(F, L, A)
    eng = pair_engine(monkeypatch, F, L, A)
    try:
        assert has_general(eng)
        eng.set_edge_mask(pair_mask(B, A))
        assert eng.template_for(B) == "pair"
        got = eng.drift(x, T, cond)
        assert np.isfinite(got).all()
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
            assert rel_l2(got[b:b + 1], orc.drift(xb, T, cb, precision=64)) < DRIFT_TOL, b
            for stage, tag in stages(L):
                _, ref = orc.drift(xb, T, cb, precision=64, tap_stage=stage)
                s, v, e = taps[tag]
                assert rel_l2(s[b:b + 1], ref["s"]) < DRIFT_TOL, (b, tag, "s")
                assert rel_l2(v[b:b + 1], ref["v"]) < DRIFT_TOL, (b, tag, "v")
                if e is not None:
                    assert rel_l2(e[b:b + 1][:, keep], ref["e"]) < DRIFT_TOL, (b, tag, "e")
    finally:
        eng.debug_tap(-1)
        eng.close()


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("F,A,L", [(32, 18, 2), (128, 18, 3), (32, 12, 3)])
def test_reruns_slices_and_stale_workspace_are_bit_identical(monkeypatch, F, A, L, masked):
    """Two runs agree bit for bit; the first eight molecules (whole groups) evaluated alone equal their rows in the batch of nine; with
    the accumulators, the edge state and the parked geometry filled with NaN, then 1e30, the result does not move: no general row
    reads an accumulator before a tile slot of its atom has replaced it, and padding rows read and write nothing."""
    _, _, _, _, x, cond = model(F, L, A)
    B = max(BATCHES)
    eng = pair_engine(monkeypatch, F, L, A)
    try:
        assert has_general(eng)
        mask = pair_mask(B, A) if masked else None
        if masked:
            eng.set_edge_mask(mask)
        ref = eng.drift(x, T, cond)
        assert np.isfinite(ref).all()
        np.testing.assert_array_equal(eng.drift(x, T, cond), ref)
        for poison in (float("nan"), 1e30):
            eng.debug_poison(B, poison)
            np.testing.assert_array_equal(eng.drift(x, T, cond), ref)
        if masked:
            eng.set_edge_mask(mask[:8])
        eng.debug_poison(B, float("nan"))
        np.testing.assert_array_equal(eng.drift(x[:8], T, cond[:8]), ref[:8])
    finally:
        eng.close()


@pytest.mark.parametrize("F", [32, 128])
def test_table_path_equals_fallback_bit_for_bit(monkeypatch, F):
    """Six cond classes round-robin over nine molecules: a general block mixes classes inside a lane."""
    A, L, B = 18, 2, 9
    _, _, _, _, x, _ = model(F, L, A)
    cond = np.empty((B, A, 2), np.float32)
    cond[..., 0] = 1000.0
    cond[..., 1] = (300.0 + 37.5 * (np.arange(B) % 6))[:, None]
    tab, fb = pair_engine(monkeypatch, F, L, A), pair_engine(monkeypatch, F, L, A, table=False)
    try:
        assert has_general(tab) and has_general(fb)
        got, ref = tab.drift(x, T, cond), fb.drift(x, T, cond)
        assert tab.debug_phi0_path() == (1, 6) and fb.debug_phi0_path() == (0, 0)
        assert np.isfinite(ref).all()
        np.testing.assert_array_equal(got, ref)
    finally:
        tab.close(); fb.close()


def test_eight_wave_build(monkeypatch):
    """8194 molecules are 2049 groups: the 8-wave tile and general builds.  They round like the 4-wave builds that serve a slice."""
    F, L, A = 32, 2, 18
    ti = pkg()
    src, dst, et = model(F, L, A)[:3]
    x, cond = ti.synthetic.molecule_coords(WIDE_B, A, seed=2), ti.synthetic.ambient_cond(WIDE_B, A)
    eng = pair_engine(monkeypatch, F, L, A)
    try:
        assert has_general(eng) and eng.template_for(WIDE_B) == "pair"
        ref = eng.drift(x, T, cond)
        assert np.isfinite(ref).all()
        np.testing.assert_array_equal(eng.drift(x, T, cond), ref)
        for lo in (0, 4096):
            np.testing.assert_array_equal(eng.drift(x[lo:lo + 8], T, cond[lo:lo + 8]), ref[lo:lo + 8])
        idx = np.r_[0:3, WIDE_B - 3:WIDE_B]
        orc = make_oracle(F, L, A, src, dst, et)
        assert rel_l2(ref[idx], orc.drift(x[idx], T, cond[idx], precision=64)) < DRIFT_TOL
    finally:
        eng.close()


def test_packed_against_the_tile_template(monkeypatch):
    """The packed template, the tile-only template and the directed layout order the same fp32 per-atom sums three ways.  The distance
    between the last two, measured here, is what one reordering costs; the packed template may sit at most twice that from the tile
    one (one more reordering)."""
    F, L, A, B = 128, 3, 18, 9
    _, _, _, _, x, cond = model(F, L, A)
    out = {}
    for name, kw in (("packed", {}), ("tile", {"packed": False}), ("directed", {"packed": False, "layout": "throughput"})):
        eng = pair_engine(monkeypatch, F, L, A, **kw)
        try:
            assert has_general(eng) == (name == "packed")
            out[name] = eng.drift(x, T, cond)
        finally:
            eng.close()
    ref = rel_l2(out["tile"], out["directed"])
    got = rel_l2(out["packed"], out["tile"])
    print(f"packed vs tile {got:.3e}; tile vs directed {ref:.3e}")
    assert np.isfinite(out["packed"]).all() and ref > 0.0 and got <= 2.0 * ref
