"""Seeded accumulators of the pair-major message kernel on the GPU (csrc/painn_pair_kernel.hpp: the SEEDED builds).
The packed template of the complete graph on 18 atoms is seeded: its general rows -- the twin pairs (2a, 2a + 1) -- name every atom of
a group exactly once.  A seeded handle runs the general launch of a layer FIRST, writing each twin message into its atom's dsacc /
dvacc rows with plain stores, then the tile launch, whose slot sums only add.  TI_PAIR_SEEDED=0 when the handle is created keeps the
order of before (tiles with first touch, then general rows that add).  The seeded path exists at A = 18 only, for plain f16x2 batches:
f32 handles, an edge mask and mixed species keep the path of before, and say so through the debug reporter.
Batches: one group (4), ragged last groups (5 and 7: one and three molecules), 1027 (257 groups, the 4-wave builds over many
workgroups) and 8193 (2048 groups -- the threshold of the 8-wave builds -- plus a ragged tail of one molecule).
Bars: DRIFT_TOL and the rollout bar 2e-5 of tests/test_gpu_pair.py against the fp64 oracle.  Needs a real MI355X: `pytest -m gpu`.
"""
import functools

import numpy as np
import pytest

from conftest import pkg, rel_l2
from oracle import oracle
from test_gpu_parity import DRIFT_TOL

pytestmark = pytest.mark.gpu

A = 18
T = 0.4
BATCHES = (4, 5, 7, 1027, 8193)
BIG = max(BATCHES)
ROLLOUT_TOL = 2e-5                           # tests/test_gpu_pair.py: test_pair_rollout_vs_reference_trajectory
SHAPES = [(32, 2), (32, 5), (128, 2), (128, 5)]


@functools.lru_cache(maxsize=None)
def model(F, L):
    ti = pkg()
    syn, W = ti.synthetic, ti.weights
    src, dst, et = syn.fully_connected_template(A)
    flat = W.flatten_state_dict(syn.painn_state_dict(0, F, L, 25, seed=F + A), W.painn_param_spec(0, F, L, 25))
    x, cond = syn.molecule_coords(BIG, A, seed=A), syn.ambient_cond(BIG, A)
    for a in (src, dst, et, flat, x, cond):
        a.setflags(write=False)
    return src, dst, et, flat, x, cond


@functools.lru_cache(maxsize=None)
def the_oracle(F, L):
    src, dst, et, flat = model(F, L)[:4]
    return oracle.PainnOracle(0, F, L, A, src, dst, et, np.arange(A), flat, temp_length=100.0)


def chunks_of_six(B):
    """up to six molecules of a batch as contiguous index ranges: the first three and the last three"""
    return [(0, min(3, B))] + ([(max(3, B - 3), B)] if B > 3 else [])


@functools.lru_cache(maxsize=None)
def oracle_drift(F, L, B):
    x, cond = model(F, L)[4:]
    out = [the_oracle(F, L).drift(x[lo:hi], T, cond[lo:hi], precision=64) for lo, hi in chunks_of_six(B)]
    for a in out:
        a.setflags(write=False)
    return out


def engine(monkeypatch, F, L, precision="f16x2", seeded=True, layout="pair"):
    """A handle with `layout` pinned.  seeded = False: created with TI_PAIR_SEEDED=0 (first-touch tiles, then general rows that add)."""
    ti = pkg()
    src, dst, et, flat = model(F, L)[:4]
    for name in ("TI_TEMPLATE", "TI_PAIR_PACKED", "TI_PHI0_TABLE", "TI_ZERO_ACC", "TI_PAIR_SEEDED"):
        monkeypatch.delenv(name, raising=False)
    if not seeded:
        monkeypatch.setenv("TI_PAIR_SEEDED", "0")
    eng = ti.engine.PainnEngine(0, F, L, A, src, dst, et, np.arange(A), flat, temp_length=100.0, precision=precision)
    monkeypatch.delenv("TI_PAIR_SEEDED", raising=False)
    eng.set_template(layout)
    return eng


def test_reporter(monkeypatch):
    on, off, f32 = engine(monkeypatch, 32, 2), engine(monkeypatch, 32, 2, seeded=False), engine(monkeypatch, 32, 2, precision="f32")
    try:
        x, cond = model(32, 2)[4:]
        assert on.debug_pair_blocks() == off.debug_pair_blocks() == (4, 39, 36) and f32.debug_pair_blocks() == (4, 45, 45)
        assert on.debug_pair_seeded() == (-1, 1) and off.debug_pair_seeded() == (-1, 1) and f32.debug_pair_seeded() == (-1, 0)
        for e in (on, off, f32):
            e.drift(x[:5], T, cond[:5])
        assert on.debug_pair_seeded() == (1, 1) and off.debug_pair_seeded() == (0, 1) and f32.debug_pair_seeded() == (0, 0)
        on.set_template("throughput")                        # the directed kernels know no seeding
        on.drift(x[:5], T, cond[:5])
        assert on.debug_pair_seeded() == (0, 1)
    finally:
        on.close(); off.close(); f32.close()


@pytest.mark.parametrize("F,L", SHAPES)
def test_drift_and_em_rollout_against_the_fp64_oracle(monkeypatch, F, L):
    x, cond = model(F, L)[4:]
    grid = pkg().engine.time_grid(0.0, 1.0, 4)               # three EM steps
    eng, orc = engine(monkeypatch, F, L), the_oracle(F, L)
    try:
        for B in BATCHES:
            got = eng.drift(x[:B], T, cond[:B])
            assert eng.debug_pair_seeded() == (1, 1) and np.isfinite(got).all()
            path, nfe = eng.rollout(x[:B], cond[:B], grid, scheme="em", eps=0.01, seed=7)
            assert nfe == 3 and eng.debug_pair_seeded() == (1, 1) and np.isfinite(path).all()
            for (lo, hi), ref in zip(chunks_of_six(B), oracle_drift(F, L, B)):
                err = rel_l2(got[lo:hi], ref)
                rp, _ = orc.rollout(x[lo:hi], cond[lo:hi], grid, scheme="em", eps=0.01, seed=7, traj_offset=lo, precision=64)
                rerr = rel_l2(path[:, lo:hi] - path[0, lo:hi], rp - rp[0])
                print(f"F {F} L {L} B {B} molecules {lo}:{hi}: drift rel-L2 {err:.2e}, EM rollout rel-L2 {rerr:.2e}")
                assert err < DRIFT_TOL, (B, lo, err)
                assert rerr < ROLLOUT_TOL, (B, lo, rerr)
    finally:
        eng.close()


@pytest.mark.parametrize("F,L", SHAPES)
def test_reruns_slices_and_poisoned_accumulators_are_bit_identical(monkeypatch, F, L):
    """Two runs agree bit for bit; whole groups evaluated alone (4-wave builds) equal their rows inside the large batch (8-wave builds);
    with dsacc / dvacc / cacc (and the edge state, the parked geometry) filled with NaN, then 1e30, nothing moves: the general launch
    stores every element of dsacc / dvacc of every atom of the batch before a tile block adds to it."""
    x, cond = model(F, L)[4:]
    eng = engine(monkeypatch, F, L)
    try:
        for B in BATCHES:
            ref = eng.drift(x[:B], T, cond[:B])
            assert np.isfinite(ref).all() and eng.debug_pair_seeded() == (1, 1)
            np.testing.assert_array_equal(eng.drift(x[:B], T, cond[:B]), ref)
            for poison in (float("nan"), 1e30):
                eng.debug_poison(B, poison)
                np.testing.assert_array_equal(eng.drift(x[:B], T, cond[:B]), ref)
            if B == BIG:
                for lo, hi in ((0, 8), (4096, 4100), (8188, 8192)):
                    eng.debug_poison(BIG, float("nan"))
                    np.testing.assert_array_equal(eng.drift(x[lo:hi], T, cond[lo:hi]), ref[lo:hi])
    finally:
        eng.close()


@pytest.mark.parametrize("F,L", SHAPES)
def test_seeded_against_the_order_of_before(monkeypatch, F, L):
    """Seeding moves a twin message from the end of an atom's fp32 sum to its start.  The pair layout and the directed layout order
    the same sums differently as well; their distance, measured here on the same inputs, bounds what the new order may cost: the
    largest |seeded - unseeded| over the test's batches must not exceed the largest |pair - directed| over the same batches.
    Both are maxima of rounding differences of a few ulps, so the comparison means something only over many elements: the figures of
    every batch are printed, the largest of each side is compared.  (Batch by batch the order of the two maxima is chance on a
    handful of molecules: at F = 32, L = 2, B = 4 -- 216 numbers -- a run gave 3.73e-08 against 3.35e-08, five against four and a
    half ulps of 2^-27.)"""
    x, cond = model(F, L)[4:]
    on, off = engine(monkeypatch, F, L), engine(monkeypatch, F, L, seeded=False)
    try:
        got, bound = [], []
        for B in BATCHES:
            a, b = on.drift(x[:B], T, cond[:B]), off.drift(x[:B], T, cond[:B])
            assert on.debug_pair_seeded() == (1, 1) and off.debug_pair_seeded() == (0, 1)
            off.set_template("throughput")
            d = off.drift(x[:B], T, cond[:B])
            off.set_template("pair")
            assert np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(d).all()
            got.append(float(np.abs(a - b).max())); bound.append(float(np.abs(b - d).max()))
            print(f"F {F} L {L} B {B}: seeded vs unseeded max |diff| {got[-1]:.3e} (rel-L2 {rel_l2(a, b):.2e}); "
                  f"pair vs directed {bound[-1]:.3e} (rel-L2 {rel_l2(b, d):.2e})")
        assert max(bound) > 0.0 and max(got) <= max(bound), (got, bound)
    finally:
        on.close(); off.close()


@pytest.mark.parametrize("F,L", [(32, 2), (128, 5)])
def test_f32_and_masked_handles_keep_the_path_of_before(monkeypatch, F, L):
    """An f32 handle and a handle with an edge mask report the unseeded path, and TI_PAIR_SEEDED changes nothing for them: bit for bit
    the result of a handle created with TI_PAIR_SEEDED=0, which runs the launches of before."""
    B = 7
    x, cond = model(F, L)[4:]
    mask = np.full((B, A), (1 << A) - 1, np.uint32)
    for a in range(A):
        mask[:, a] &= ~np.uint32(1 << a)
    for b in range(B):                                       # molecule b loses the pair (b, b + 1): a twin pair for even b
        mask[b, b] &= ~np.uint32(1 << (b + 1))
        mask[b, b + 1] &= ~np.uint32(1 << b)
    for precision, masked in (("f32", False), ("f16x2", True)):
        on, off = engine(monkeypatch, F, L, precision), engine(monkeypatch, F, L, precision, seeded=False)
        try:
            if masked:
                on.set_edge_mask(mask); off.set_edge_mask(mask)
            a, b = on.drift(x[:B], T, cond[:B]), off.drift(x[:B], T, cond[:B])
            assert on.debug_pair_seeded()[0] == 0 and off.debug_pair_seeded()[0] == 0
            assert on.template_for(B) == "pair" and np.isfinite(a).all()
            np.testing.assert_array_equal(a, b)
            if masked:                                       # without the mask the same handle is seeded again
                on.set_edge_mask(None)
                plain = on.drift(x[:B], T, cond[:B])
                assert on.debug_pair_seeded() == (1, 1)
                # a mask that removes nothing leaves the template's rows: the launches, and the bits, of the unmasked batch
                on.set_edge_mask(np.full((B, A), (1 << A) - 1, np.uint32))
                np.testing.assert_array_equal(on.drift(x[:B], T, cond[:B]), plain)
                assert on.debug_pair_seeded() == (1, 1)
        finally:
            on.close(); off.close()
