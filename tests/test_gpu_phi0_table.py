"""The layer-0 phi table (csrc/painn_phi0_kernels.hip, the TABLE builds of csrc/painn_pair_kernel.hpp): entering the
first message layer the phi branch does not see the coordinates, so it is evaluated once per (cond class, atom, edge type) and the
pair kernel reads the result.  Every table entry is the value the kernel would have computed, so a drift or rollout on the table path
must equal the fallback (TI_PHI0_TABLE=0 when the handle is created) BIT FOR BIT; the getter says which path an evaluation took.
Needs a real MI355X: `pytest -m gpu`.
"""
import functools

import numpy as np
import pytest

from conftest import pkg, rel_l2
from oracle import oracle
from test_gpu_parity import DRIFT_TOL

pytestmark = pytest.mark.gpu

CAP = 16            # include/ti_hip.h TI_PHI0_MAX_CLASSES
T = 0.4


@functools.lru_cache(maxsize=None)
def model(F, L, A, B):
    ti = pkg()
    syn, W = ti.synthetic, ti.weights
    src, dst, et = syn.fully_connected_template(A)
    flat = W.flatten_state_dict(syn.painn_state_dict(0, F, L, 25, seed=F + A), W.painn_param_spec(0, F, L, 25))
    x, cond = syn.molecule_coords(B, A, seed=A), syn.ambient_cond(B, A)          # T1 round-robin over a 6-rung ladder
    for a in (src, dst, et, flat, x, cond):
        a.setflags(write=False)
    return src, dst, et, flat, x, cond


def engine(monkeypatch, F, L, A, table, precision="f16x2"):
    """A handle with the pair layout pinned; table = False: created with TI_PHI0_TABLE=0 (the kernels of before)."""
    ti = pkg()
    src, dst, et, flat = model(F, L, A, 1)[:4]
    monkeypatch.setenv("TI_TEMPLATE", "pair")
    if table:
        monkeypatch.delenv("TI_PHI0_TABLE", raising=False)
    else:
        monkeypatch.setenv("TI_PHI0_TABLE", "0")
    eng = ti.engine.PainnEngine(0, F, L, A, src, dst, et, np.arange(A), flat, temp_length=100.0, precision=precision)
    monkeypatch.delenv("TI_PHI0_TABLE", raising=False)
    return eng


def class_cond(B, A, classes, order="round_robin", seed=0):
    """[B, A, 2]: T0 = 1000, T1 one of `classes` values; which molecule gets which: round-robin, shuffled, or sorted into runs."""
    ids = np.arange(B) % classes
    if order == "shuffled":
        ids = np.random.default_rng(seed).permutation(ids)
    elif order == "sorted":
        ids = np.sort(ids)
    c = np.empty((B, A, 2), np.float32)
    c[..., 0] = 1000.0
    c[..., 1] = (300.0 + 37.5 * ids)[:, None]
    return c


def both(monkeypatch, F, L, A, precision="f16x2"):
    return engine(monkeypatch, F, L, A, True, precision), engine(monkeypatch, F, L, A, False, precision)


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("A", [18, 5, 3])
@pytest.mark.parametrize("F", [32, 128])
def test_table_path_equals_fallback_bit_for_bit(monkeypatch, F, A, L):
    """drift and a 3-step EM rollout (t moves every step: a stale table would show) at B = 4, 6 (the last group reaches past the
    batch) and 13; A = 18 has loose blocks and the 2-atom tile, A = 5 and 3 mostly absent rows."""
    ti = pkg()
    x13, cond13 = model(F, L, A, 13)[4:]
    tab, fb = both(monkeypatch, F, L, A)
    grid = ti.engine.time_grid(0.0, 1.0, 4)
    try:
        for B in (4, 6, 13):
            x, cond = x13[:B], cond13[:B]
            assert tab.template_for(B) == "pair" and fb.template_for(B) == "pair"
            got, ref = tab.drift(x, T, cond), fb.drift(x, T, cond)
            assert tab.debug_phi0_path() == (1, min(B, 6)) and fb.debug_phi0_path() == (0, 0)
            assert np.isfinite(ref).all()
            np.testing.assert_array_equal(got, ref)
            pg, ng = tab.rollout(x, cond, grid, scheme="em", eps=0.01, seed=7)
            pr, nr = fb.rollout(x, cond, grid, scheme="em", eps=0.01, seed=7)
            assert ng == nr == 3 and tab.debug_phi0_path()[0] == 1 and fb.debug_phi0_path()[0] == 0
            np.testing.assert_array_equal(pg, pr)
    finally:
        tab.close(); fb.close()


CLASS_CASES = {
    "one": lambda B, A: (class_cond(B, A, 1), 1),
    "six_round_robin": lambda B, A: (class_cond(B, A, 6), 6),                 # groups and loose blocks mix classes
    "six_shuffled": lambda B, A: (class_cond(B, A, 6, "shuffled", 3), 6),
    "six_sorted": lambda B, A: (class_cond(B, A, 6, "sorted"), 6),
    "cap": lambda B, A: (class_cond(B, A, CAP, "shuffled", 5), CAP),
    "cap_plus_one": lambda B, A: (class_cond(B, A, CAP + 1, "shuffled", 6), CAP + 1),
}


@pytest.mark.parametrize("case", list(CLASS_CASES) + ["one_atom_differs"])
def test_classes_whatever_the_order(monkeypatch, case):
    F, L, A, B = 32, 2, 18, 40
    x = model(F, L, A, B)[4]
    if case == "one_atom_differs":                # one molecule differs from the rest in a single atom's T1, by one ulp
        cond, n = class_cond(B, A, 1), 2
        cond[7, 3, 1] = np.nextafter(cond[7, 3, 1], np.float32(2000.0))
    else:
        cond, n = CLASS_CASES[case](B, A)
    tab, fb = both(monkeypatch, F, L, A)
    try:
        got, ref = tab.drift(x, T, cond), fb.drift(x, T, cond)
        assert tab.debug_phi0_path() == ((1, n) if n <= CAP else (0, CAP + 1))     # more classes than the cap: the fallback, reported
        assert np.isfinite(ref).all()
        np.testing.assert_array_equal(got, ref)
    finally:
        tab.close(); fb.close()


def test_cond_then_time_change_on_one_handle(monkeypatch):
    """Nothing of an earlier call survives: other classes in the second drift, another t in the third."""
    F, L, A, B = 32, 2, 18, 13
    x = model(F, L, A, B)[4]
    tab, fb = both(monkeypatch, F, L, A)
    try:
        for cond, t, n in ((class_cond(B, A, 6), T, 6), (class_cond(B, A, 3, "shuffled", 1) + np.float32(12.5), T, 3), (class_cond(B, A, 3, "shuffled", 1) + np.float32(12.5), 0.9, 3)):
            got, ref = tab.drift(x, t, cond), fb.drift(x, t, cond)
            assert tab.debug_phi0_path() == (1, n)
            np.testing.assert_array_equal(got, ref)
    finally:
        tab.close(); fb.close()


def test_fallbacks_report_themselves_and_change_nothing(monkeypatch):
    """Per-molecule times, an edge mask, a ragged handle and a debug tap keep the kernels of before: path 0, and the bits of a handle
    created with TI_PHI0_TABLE=0."""
    F, L, A, B = 32, 2, 18, 9
    x, cond = model(F, L, A, B)[4:]
    tab, fb = both(monkeypatch, F, L, A)
    try:
        np.testing.assert_array_equal(tab.drift(x, T, cond), fb.drift(x, T, cond))
        assert tab.debug_phi0_path()[0] == 1
        tv = np.linspace(0.1, 0.9, B).astype(np.float32)
        np.testing.assert_array_equal(tab.drift(x, tv, cond), fb.drift(x, tv, cond))
        assert tab.debug_phi0_path() == (0, 0)
        mask = np.array([[((1 << A) - 1) & ~(1 << d) for d in range(A)]] * B, np.uint32)        # bit s of mask[b, d]: edge s -> d
        mask[2, 1] &= ~np.uint32(1 << 4); mask[2, 4] &= ~np.uint32(1 << 1)             # molecule 2 loses the pair (1, 4), both directions
        for e in (tab, fb):
            e.set_edge_mask(mask)
        np.testing.assert_array_equal(tab.drift(x, T, cond), fb.drift(x, T, cond))
        assert tab.debug_phi0_path() == (0, 0)
        n_atoms = np.full(B, A, np.int32); n_atoms[3] = A - 2
        for e in (tab, fb):
            e.set_molecules(n_atoms)
        np.testing.assert_array_equal(tab.drift(x, T, cond), fb.drift(x, T, cond))
        assert tab.debug_phi0_path() == (0, 0)
        for e in (tab, fb):
            e.set_molecules(None)
            e.debug_tap(1)
            e.drift(x, T, cond)
        assert tab.debug_phi0_path() == (0, 0)
        np.testing.assert_array_equal(tab.debug_read("s", B), fb.debug_read("s", B))
        np.testing.assert_array_equal(tab.debug_read("e", B), fb.debug_read("e", B))
        for e in (tab, fb):
            e.debug_tap(-1)
        np.testing.assert_array_equal(tab.drift(x, T, cond), fb.drift(x, T, cond))       # and back on the table
        assert tab.debug_phi0_path() == (1, 6)
    finally:
        for e in (tab, fb):
            e.debug_tap(-1)
            e.close()


def test_f32_has_no_table_build(monkeypatch):
    F, L, A, B = 32, 2, 18, 9
    x, cond = model(F, L, A, B)[4:]
    tab, fb = both(monkeypatch, F, L, A, precision="f32")
    try:
        np.testing.assert_array_equal(tab.drift(x, T, cond), fb.drift(x, T, cond))
        assert tab.debug_phi0_path() == (0, 0)
    finally:
        tab.close(); fb.close()


def test_eight_wave_build(monkeypatch):
    """2 049 groups: the 8-wave build.  The whole batch equals the fallback; two whole groups evaluated alone (the 4-wave build)
    equal their rows in the batch."""
    F, L, A, B = 32, 2, 18, 8194
    x, cond = model(F, L, A, B)[4:]
    tab, fb = both(monkeypatch, F, L, A)
    try:
        got = tab.drift(x, T, cond)
        assert tab.debug_phi0_path() == (1, 6)
        np.testing.assert_array_equal(got, fb.drift(x, T, cond))
        np.testing.assert_array_equal(tab.drift(x[:8], T, cond[:8]), got[:8])
        np.testing.assert_array_equal(tab.drift(x[4096:4104], T, cond[4096:4104]), got[4096:4104])
    finally:
        tab.close(); fb.close()


def test_poisoned_workspace(monkeypatch):
    """NaN, then 1e30, in the accumulators, the edge state, the parked geometry and the table before the call: nothing moves."""
    F, L, A, B = 128, 3, 18, 9
    x, cond = model(F, L, A, B)[4:]
    tab = engine(monkeypatch, F, L, A, True)
    try:
        ref = tab.drift(x, T, cond)
        assert np.isfinite(ref).all() and tab.debug_phi0_path() == (1, 6)
        for poison in (float("nan"), 1e30):
            tab.debug_poison(B, poison)
            np.testing.assert_array_equal(tab.drift(x, T, cond), ref)
            assert tab.debug_phi0_path() == (1, 6)
    finally:
        tab.close()


def test_table_path_against_the_fp64_oracle(monkeypatch):
    """The bar of tests/test_gpu_pair_outstage.py (DRIFT_TOL) on the table path: 6 molecules, A = 18, F = 128."""
    F, L, A, B = 128, 3, 18, 6
    src, dst, et, flat, x, cond = model(F, L, A, B)
    tab = engine(monkeypatch, F, L, A, True)
    orc = oracle.PainnOracle(0, F, L, A, src, dst, et, np.arange(A), flat, temp_length=100.0)
    try:
        got = tab.drift(x, T, cond)
        err = rel_l2(got, orc.drift(x, T, cond, precision=64))
        print(f"table path, F {F} A {A} L {L} B {B}: drift rel-L2 {err:.2e}")
        assert tab.debug_phi0_path() == (1, 6)
        assert np.isfinite(got).all() and err < DRIFT_TOL, err
    finally:
        tab.close()
