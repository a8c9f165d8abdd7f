"""Embed per class on the phi table path (csrc/painn_kernels.hip: painn_embed16_cls_kernel, painn_update_cls_kernel).
On that path the embedding has two readers -- the table kernel (P of the class representatives) and layer 0's update (s, once) -- and
the rows of a class agree bit for bit, so the embed launch covers (class, atom) rows alone and layer 0's update reads s through the
class map.  TI_EMBED_CLASSES=0 when the handle is created keeps the embed launch over every atom: drift and rollout must equal that
handle's BIT FOR BIT, also with the full s / P (which such an evaluation must not read before layer 0's update wrote them) poisoned.
More classes than the cap fall back, and say so.  Needs a real MI355X: `pytest -m gpu`.
"""
import functools

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

CAP = 16            # include/ti_hip.h TI_PHI0_MAX_CLASSES
A = 18
T = 0.4
B_MAX = 70          # 17 groups of 4 and a half: B is no multiple of G in any case below
SWITCHES = ("TI_TEMPLATE", "TI_PAIR_PACKED", "TI_PHI0_TABLE", "TI_ZERO_ACC", "TI_PAIR_SEEDED", "TI_PAIR_TAILS", "TI_EMBED_CLASSES")


@functools.lru_cache(maxsize=None)
def model(F, L):
    ti = pkg()
    syn, W = ti.synthetic, ti.weights
    src, dst, et = syn.fully_connected_template(A)
    flat = W.flatten_state_dict(syn.painn_state_dict(0, F, L, 25, seed=F + A), W.painn_param_spec(0, F, L, 25))
    x = syn.molecule_coords(B_MAX, A, seed=A)
    for a in (src, dst, et, flat, x):
        a.setflags(write=False)
    return src, dst, et, flat, x


def engine(monkeypatch, F, L, per_class):
    """A handle with the pair layout pinned; per_class = False: created with TI_EMBED_CLASSES=0 (the embed launch over every atom)."""
    ti = pkg()
    src, dst, et, flat = model(F, L)[:4]
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if not per_class:
        monkeypatch.setenv("TI_EMBED_CLASSES", "0")
    eng = ti.engine.PainnEngine(0, F, L, A, src, dst, et, np.arange(A), flat, temp_length=100.0, precision="f16x2")
    monkeypatch.delenv("TI_EMBED_CLASSES", raising=False)
    eng.set_template("pair")
    return eng


def class_cond(B, classes, order="round_robin", seed=0):
    """[B, A, 2]: T0 = 1000, T1 one of `classes` values; which molecule gets which: round-robin or shuffled"""
    ids = np.arange(B) % classes
    if order == "shuffled":
        ids = np.random.default_rng(seed).permutation(ids)
    c = np.empty((B, A, 2), np.float32)
    c[..., 0] = 1000.0
    c[..., 1] = (300.0 + 37.5 * ids)[:, None]
    return c


CASES = {                                   # (classes, order, B): B never a multiple of G = 4
    "one": (1, "round_robin", 13),
    "six_round_robin": (6, "round_robin", 13),
    "six_shuffled": (6, "shuffled", 41),
    "cap_shuffled": (CAP, "shuffled", B_MAX),
    "cap_plus_one": (CAP + 1, "shuffled", B_MAX),
}


def test_reporter(monkeypatch):
    F, L = 32, 2
    x = model(F, L)[4]
    on, off = engine(monkeypatch, F, L, True), engine(monkeypatch, F, L, False)
    try:
        assert on.debug_embed_path() == -1 and off.debug_embed_path() == -1
        cond = class_cond(13, 6)
        on.drift(x[:13], T, cond); off.drift(x[:13], T, cond)
        assert on.debug_phi0_path() == (1, 6) and off.debug_phi0_path() == (1, 6)         # both on the table; only the embed launch differs
        assert on.debug_embed_path() == 1 and off.debug_embed_path() == 0
        on.set_template("throughput")                            # off the table path: the embed launch of before
        on.drift(x[:13], T, cond)
        assert on.debug_phi0_path()[0] == 0 and on.debug_embed_path() == 0
    finally:
        on.close(); off.close()


@pytest.mark.parametrize("F,L", [(32, 1), (32, 2), (128, 5)])
@pytest.mark.parametrize("case", list(CASES))
def test_drift_and_rollout_equal_the_full_embed_bit_for_bit(monkeypatch, case, F, L):
    """drift and a 3-step EM rollout (t moves every step: stale class rows would show), plain and with the workspace poisoned -- the
    full s / P among it -- with NaN, then 1e30, before the call."""
    classes, order, B = CASES[case]
    ti = pkg()
    x, cond = model(F, L)[4][:B], class_cond(B, classes, order, seed=5)
    grid = ti.engine.time_grid(0.0, 1.0, 4)
    on, off = engine(monkeypatch, F, L, True), engine(monkeypatch, F, L, False)
    try:
        ref = off.drift(x, T, cond)
        assert np.isfinite(ref).all() and off.debug_embed_path() == 0
        want = 1 if classes <= CAP else 0                        # more classes than the cap: the fallback, reported
        for poison in (None, float("nan"), 1e30):
            if poison is not None:
                on.debug_poison(B_MAX, poison)
            got = on.drift(x, T, cond)
            assert on.debug_phi0_path() == ((1, classes) if classes <= CAP else (0, CAP + 1)) and on.debug_embed_path() == want
            np.testing.assert_array_equal(got, ref)
        pr, nr = off.rollout(x, cond, grid, scheme="em", eps=0.01, seed=7)
        for poison in (None, float("nan")):
            if poison is not None:
                on.debug_poison(B_MAX, poison)
            pg, ng = on.rollout(x, cond, grid, scheme="em", eps=0.01, seed=7)
            assert ng == nr == 3 and on.debug_embed_path() == want
            np.testing.assert_array_equal(pg, pr)
    finally:
        on.close(); off.close()


def test_classes_change_between_calls_on_one_handle(monkeypatch):
    """Nothing of an earlier call's class rows survives: other classes in the second drift, another t in the third, then a call off
    the table path (17 classes) and back."""
    F, L, B = 32, 2, 41
    x = model(F, L)[4][:B]
    on, off = engine(monkeypatch, F, L, True), engine(monkeypatch, F, L, False)
    try:
        for classes, shift, t in ((6, 0.0, T), (3, 12.5, T), (3, 12.5, 0.9), (CAP + 1, 0.0, T), (2, 0.0, T)):
            cond = class_cond(B, classes, "shuffled", seed=classes) + np.float32(shift)
            got, ref = on.drift(x, t, cond), off.drift(x, t, cond)
            assert on.debug_embed_path() == (1 if classes <= CAP else 0)
            np.testing.assert_array_equal(got, ref)
    finally:
        on.close(); off.close()
