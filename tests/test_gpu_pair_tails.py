"""Merged tails of the seeded general launch on the GPU (csrc/painn_pair_kernel.hpp: painn_pair_general_tails_kernel).
The packed template of K18 at G = 4 ends with general blocks of 16, 16 and 4 valid rows.  With merged tails one wave owns a super-group
of S = 4 groups: it walks their full general blocks, then their four last blocks as ONE block of 16 rows -- 9 blocks per 4 groups
instead of 12.  Storage and row words stay; a row's value does not depend on its block mates; seeds are plain stores.  So drift and
rollout must equal those of a handle created with TI_PAIR_TAILS=0 (one group per wave) BIT FOR BIT -- layer 0 on and off the phi
table, with the edge state, the parks and the accumulators poisoned, and for a slice of whole super-groups evaluated alone.
Batches: 16 (one super-group), 13 and 17 (a partial group inside a super-group; a partial super-group of one partial group), 64, and
8193 (2049 groups: the 8-wave builds run from 2048 groups; 513 super-groups, the last of one molecule).
Bars against the fp64 oracle: DRIFT_TOL and the rollout bar 2e-5 of tests/test_gpu_pair_seeded.py.  Needs a real MI355X: `pytest -m gpu`.
"""
import functools

import numpy as np
import pytest

from conftest import pkg, rel_l2
from oracle import oracle
from test_gpu_parity import DRIFT_TOL

pytestmark = pytest.mark.gpu

A = 18
F = 32
T = 0.4
BATCHES = (16, 13, 17, 64, 8193)
BIG = max(BATCHES)
ROLLOUT_TOL = 2e-5                           # tests/test_gpu_pair_seeded.py
LAYERS = (2, 5)
SWITCHES = ("TI_TEMPLATE", "TI_PAIR_PACKED", "TI_PHI0_TABLE", "TI_ZERO_ACC", "TI_PAIR_SEEDED", "TI_PAIR_TAILS", "TI_EMBED_CLASSES")


@functools.lru_cache(maxsize=None)
def model(L):
    ti = pkg()
    syn, W = ti.synthetic, ti.weights
    src, dst, et = syn.fully_connected_template(A)
    flat = W.flatten_state_dict(syn.painn_state_dict(0, F, L, 25, seed=F + A), W.painn_param_spec(0, F, L, 25))
    x, cond = syn.molecule_coords(BIG, A, seed=A), syn.ambient_cond(BIG, A)           # T1 round-robin over a 6-rung ladder: 6 classes
    for a in (src, dst, et, flat, x, cond):
        a.setflags(write=False)
    return src, dst, et, flat, x, cond


@functools.lru_cache(maxsize=None)
def the_oracle(L):
    src, dst, et, flat = model(L)[:4]
    return oracle.PainnOracle(0, F, L, A, src, dst, et, np.arange(A), flat, temp_length=100.0)


def chunks_of_six(B):
    """six molecules of a batch as contiguous index ranges: the first three and the last three"""
    return [(0, 3), (B - 3, B)]


def engine(monkeypatch, L, tails, table):
    """A handle with the pair layout pinned.  tails = False: created with TI_PAIR_TAILS=0 (one group per wave); table = False: created
    with TI_PHI0_TABLE=0 (layer 0 computes its phi branch)."""
    ti = pkg()
    src, dst, et, flat = model(L)[:4]
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if not tails:
        monkeypatch.setenv("TI_PAIR_TAILS", "0")
    if not table:
        monkeypatch.setenv("TI_PHI0_TABLE", "0")
    eng = ti.engine.PainnEngine(0, F, L, A, src, dst, et, np.arange(A), flat, temp_length=100.0, precision="f16x2")
    monkeypatch.delenv("TI_PAIR_TAILS", raising=False)
    monkeypatch.delenv("TI_PHI0_TABLE", raising=False)
    eng.set_template("pair")
    return eng


def test_reporter(monkeypatch):
    x, cond = model(2)[4:]
    on, off = engine(monkeypatch, 2, True, True), engine(monkeypatch, 2, False, True)
    try:
        assert on.debug_pair_blocks() == off.debug_pair_blocks() == (4, 39, 36)
        assert on.debug_pair_tails() == (-1, 4) and off.debug_pair_tails() == (-1, 4)
        on.drift(x[:13], T, cond[:13]); off.drift(x[:13], T, cond[:13])
        assert on.debug_pair_seeded() == (1, 1) and off.debug_pair_seeded() == (1, 1)           # both seeded; only the walk differs
        assert on.debug_pair_tails() == (1, 4) and off.debug_pair_tails() == (0, 4)
        on.set_template("throughput")                            # the directed kernels have no general launch
        on.drift(x[:13], T, cond[:13])
        assert on.debug_pair_tails() == (0, 4)
    finally:
        on.close(); off.close()


@pytest.mark.parametrize("table", [True, False], ids=["table", "no_table"])
@pytest.mark.parametrize("L", LAYERS)
def test_drift_and_rollout_equal_the_walk_of_one_group_per_wave_bit_for_bit(monkeypatch, L, table):
    """drift and a 3-step EM rollout of every batch; then the drift again with e, the parks and the accumulators (and the phi table,
    s and P) filled with NaN, then 1e30; at the large batch, whole super-groups (16 molecules) evaluated alone -- the 4-wave builds --
    equal their rows inside the batch -- the 8-wave builds; and six molecules per batch against the fp64 oracle."""
    x, cond = model(L)[4:]
    grid = pkg().engine.time_grid(0.0, 1.0, 4)               # three EM steps
    on, off, orc = engine(monkeypatch, L, True, table), engine(monkeypatch, L, False, table), the_oracle(L)
    try:
        for B in BATCHES:
            got, ref = on.drift(x[:B], T, cond[:B]), off.drift(x[:B], T, cond[:B])
            assert on.debug_pair_tails() == (1, 4) and off.debug_pair_tails() == (0, 4)
            assert on.debug_phi0_path()[0] == off.debug_phi0_path()[0] == (1 if table else 0)
            assert np.isfinite(ref).all()
            np.testing.assert_array_equal(got, ref)
            pg, ng = on.rollout(x[:B], cond[:B], grid, scheme="em", eps=0.01, seed=7)
            pr, nr = off.rollout(x[:B], cond[:B], grid, scheme="em", eps=0.01, seed=7)
            assert ng == nr == 3 and on.debug_pair_tails() == (1, 4) and off.debug_pair_tails() == (0, 4)
            np.testing.assert_array_equal(pg, pr)
            for poison in (float("nan"), 1e30):
                on.debug_poison(B, poison)
                np.testing.assert_array_equal(on.drift(x[:B], T, cond[:B]), ref)
            on.debug_poison(B, float("nan"))
            np.testing.assert_array_equal(on.rollout(x[:B], cond[:B], grid, scheme="em", eps=0.01, seed=7)[0], pr)
            if B == BIG:
                for lo, hi in ((0, 16), (4096, 4128), (8176, 8192)):
                    on.debug_poison(BIG, float("nan"))
                    np.testing.assert_array_equal(on.drift(x[lo:hi], T, cond[lo:hi]), ref[lo:hi])
            for lo, hi in chunks_of_six(B):
                want = orc.drift(x[lo:hi], T, cond[lo:hi], precision=64)
                err = rel_l2(got[lo:hi], want)
                rp, _ = orc.rollout(x[lo:hi], cond[lo:hi], grid, scheme="em", eps=0.01, seed=7, traj_offset=lo, precision=64)
                rerr = rel_l2(pg[:, lo:hi] - pg[0, lo:hi], rp - rp[0])
                print(f"L {L} table {table} B {B} molecules {lo}:{hi}: drift rel-L2 {err:.2e}, EM rollout rel-L2 {rerr:.2e}")
                assert err < DRIFT_TOL, (B, lo, err)
                assert rerr < ROLLOUT_TOL, (B, lo, rerr)
    finally:
        on.close(); off.close()
