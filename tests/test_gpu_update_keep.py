"""Update launches that keep v_eff in registers (csrc/painn_update_keep.hip: painn_update_keep_kernel, painn_update_cls_keep_kernel;
csrc/painn_update_kernel_body.inc: KEEP).  The update kernel forms v_eff = v + dv in its first phase and needs it
again in its last.  The builds of before park it in the dv accumulator in between; the f16x2 builds up to F = 128 have twins that keep
components of it in fp32 registers: the same values in the same expressions.  TI_UPDATE_KEEP=0 when the handle is created launches the
builds of before: drift, rollouts, the state after an update stage and the divergence must equal that handle's BIT FOR BIT, also with
the accumulators poisoned (a last phase that still loaded a component it keeps would read the poison, or the message sum instead of
v_eff).  Needs a real MI355X: `pytest -m gpu`.
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
# N = 18 B nodes, 16 to a wave, 64 to a workgroup: 18, 54, 90, 126 are multiples of neither (the last wave has absent rows), 522 is
# nine workgroups and a tail, 1152 = 18 * 64 an exact multiple
BATCHES = (1, 3, 5, 7, 29, 64)
B_MAX = max(BATCHES)
ROLLOUT_TOL = 2e-5                           # tests/test_gpu_pair_seeded.py
KEPT = {32: 2, 64: 2, 128: 2}                # csrc/painn_update_keep.hip: update_keep
SWITCHES = ("TI_TEMPLATE", "TI_PAIR_PACKED", "TI_PHI0_TABLE", "TI_ZERO_ACC", "TI_PAIR_SEEDED", "TI_PAIR_TAILS", "TI_EMBED_CLASSES", "TI_UPDATE_KEEP")


@functools.lru_cache(maxsize=None)
def model(F, L):
    ti = pkg()
    syn, W = ti.synthetic, ti.weights
    src, dst, et = syn.fully_connected_template(A)
    flat = W.flatten_state_dict(syn.painn_state_dict(0, F, L, 25, seed=F + A), W.painn_param_spec(0, F, L, 25))
    x = syn.molecule_coords(B_MAX, A, seed=A)
    cond = np.empty((B_MAX, A, 2), np.float32)               # six conditioning classes: the pair layout's layer 0 runs on the phi table
    cond[..., 0] = 1000.0
    cond[..., 1] = (300.0 + 37.5 * (np.arange(B_MAX) % 6))[:, None]
    for a in (src, dst, et, flat, x, cond):
        a.setflags(write=False)
    return src, dst, et, flat, x, cond


def engine(monkeypatch, F, L, keep, precision="f16x2", env=()):
    """A handle created with the switches of `env` ((name, value) pairs); keep = False: with TI_UPDATE_KEEP=0 (the update builds of before)."""
    ti = pkg()
    src, dst, et, flat = model(F, L)[:4]
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in env:
        monkeypatch.setenv(name, value)
    if not keep:
        monkeypatch.setenv("TI_UPDATE_KEEP", "0")
    eng = ti.engine.PainnEngine(0, F, L, A, src, dst, et, np.arange(A), flat, temp_length=100.0, precision=precision)
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return eng


def edge_mask(B):
    """every template edge but: molecule b loses the pair (b % 17, b % 17 + 1), both directions"""
    mask = np.full((B, A), (1 << A) - 1, np.uint32)
    for a in range(A):
        mask[:, a] &= ~np.uint32(1 << a)
    for b in range(B):
        i = b % (A - 1)
        mask[b, i] &= ~np.uint32(1 << (i + 1))
        mask[b, i + 1] &= ~np.uint32(1 << i)
    return mask


def compare(on, off, B, kept, setup=None):
    """drift and a 3-step EM rollout of B molecules on both handles: equal bytes, plain and with the workspace poisoned with NaN, then
    1e30, before the call.  setup(engine, B): what the case puts in force for this batch size."""
    ti = pkg()
    x, cond = model(on.F, on.L)[4:]
    x, cond = x[:B], cond[:B]
    grid = ti.engine.time_grid(0.0, 1.0, 4)
    if setup is not None:
        setup(on, B); setup(off, B)
    ref = off.drift(x, T, cond)
    assert np.isfinite(ref).all() and off.debug_update_keep() == 0
    pr, nr = off.rollout(x, cond, grid, scheme="em", eps=0.01, seed=7)
    assert nr == 3 and np.isfinite(pr).all()
    for poison in (None, float("nan"), 1e30):
        if poison is not None:
            on.debug_poison(B, poison)
        got = on.drift(x, T, cond)
        assert on.debug_update_keep() == kept
        assert got.tobytes() == ref.tobytes(), (B, poison, float(np.abs(got - ref).max()))
        if poison is not None:
            on.debug_poison(B, poison)
        pg, ng = on.rollout(x, cond, grid, scheme="em", eps=0.01, seed=7)
        assert ng == 3 and pg.tobytes() == pr.tobytes(), (B, poison)


def test_reporter(monkeypatch):
    """the kept components on a default handle, 0 on a handle of the switch and on an f32 handle, -1 before any evaluation"""
    F, L = 128, 2
    x, cond = model(F, L)[4:]
    on, off, f32 = engine(monkeypatch, F, L, True), engine(monkeypatch, F, L, False), engine(monkeypatch, F, L, True, precision="f32")
    try:
        assert on.debug_update_keep() == off.debug_update_keep() == f32.debug_update_keep() == -1
        for e in (on, off, f32):
            e.drift(x[:5], T, cond[:5])
        assert on.debug_update_keep() == KEPT[F] and off.debug_update_keep() == 0 and f32.debug_update_keep() == 0
    finally:
        on.close(); off.close(); f32.close()
    for F in (32, 64):
        on = engine(monkeypatch, F, 1, True)
        try:
            on.drift(x[:5], T, cond[:5])
            assert on.debug_update_keep() == KEPT[F]
        finally:
            on.close()


@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("F", [32, 64, 128])
def test_widths_and_depths_equal_the_parked_builds_bit_for_bit(monkeypatch, F, L):
    """L = 1: layer 0 alone (first layer and no next); L = 2: first and last; L = 3: a middle layer.  Pair layout at every batch size:
    layer 0's update is the per-class twin (the phi table), the later ones the folded builds."""
    on, off = engine(monkeypatch, F, L, True), engine(monkeypatch, F, L, False)
    try:
        on.set_template("pair"); off.set_template("pair")
        for B in BATCHES:
            compare(on, off, B, KEPT[F])
            assert on.template_for(B) == off.template_for(B) == "pair"
            assert on.debug_embed_path() == 1 and off.debug_embed_path() == 1          # painn_update_cls_keep_kernel against its twin
    finally:
        on.close(); off.close()


def _mask(e, B):
    e.set_edge_mask(edge_mask(B))


def _species(e, B):
    e.set_molecules(np.asarray([(18, 12, 5, 17, 1)[b % 5] for b in range(B)], np.int32))


PATHS = {                                      # (switches at creation, layout pinned after it, what is put in force per batch)
    "directed": ((), "throughput", None),                                # not folded: the cacc cross term inside the kept row
    "table_off": ((("TI_PHI0_TABLE", "0"),), "pair", None),              # layer 0 on painn_update_keep_kernel, not the per-class twin
    "zero_acc": ((("TI_ZERO_ACC", "1"),), "pair", None),                 # the accumulators are reset by the update, kept rows included
    "mask_pair": ((), "pair", _mask),
    "mask_directed": ((), "throughput", _mask),
    "species_pair": ((), "pair", _species),
    "species_directed": ((), "throughput", _species),
}


@pytest.mark.parametrize("F", [32, 128])
@pytest.mark.parametrize("path", list(PATHS))
def test_paths_through_the_build_matrix(monkeypatch, path, F):
    L = 3
    env, layout, setup = PATHS[path]
    on, off = engine(monkeypatch, F, L, True, env=env), engine(monkeypatch, F, L, False, env=env)
    try:
        on.set_template(layout); off.set_template(layout)
        for B in (3, 7, 29, 64):
            compare(on, off, B, KEPT[F], setup)
            assert on.template_for(B) == off.template_for(B) == layout
            if path == "table_off":
                assert on.debug_phi0_path()[0] == 0 and on.debug_embed_path() == 0
    finally:
        on.close(); off.close()


@pytest.mark.parametrize("layout", ["pair", "throughput"])
@pytest.mark.parametrize("F", [32, 128])
def test_state_after_every_update_stage(monkeypatch, F, layout):
    """The debug taps stop an evaluation after a stage and read state + pending accumulators (s + dsacc, v + dvacc + cacc x v): after
    an update stage the two handles must agree bit for bit.  A tapped evaluation has the update reset the accumulators it consumed
    (tests/test_gpu_pair_packed.py pins the taps of the parked builds against the oracle); an accumulator that a kept build left
    standing -- dvacc of a kept component holds the message sum, never v_eff -- is added into the read and shows as a difference."""
    L, B = 3, 7
    x, cond = model(F, L)[4:]
    on, off = engine(monkeypatch, F, L, True), engine(monkeypatch, F, L, False)
    try:
        on.set_template(layout); off.set_template(layout)
        for l in range(L):
            for e in (on, off):
                e.debug_tap(2 + 2 * l)
                e.drift(x[:B], T, cond[:B])
            assert on.debug_update_keep() == KEPT[F] and off.debug_update_keep() == 0
            for what in ("s", "v"):
                a, b = on.debug_read(what, B), off.debug_read(what, B)
                assert np.isfinite(b).all() and np.abs(b).max() > 0
                assert a.tobytes() == b.tobytes(), (l, what)
    finally:
        for e in (on, off):
            e.debug_tap(-1)
            e.close()


@pytest.mark.parametrize("F", [32, 128])
def test_divergence_reads_the_primal_state_around_the_update(monkeypatch, F):
    """the tangent kernels read dvacc before the update and v after it: one exact divergence of three molecules on both handles"""
    L, B = 3, 3
    x, cond = model(F, L)[4:]
    on, off = engine(monkeypatch, F, L, True), engine(monkeypatch, F, L, False)
    try:
        for poison in (None, float("nan")):
            if poison is not None:
                on.debug_poison(B, poison)
            (b1, d1), (b0, d0) = on.drift_div(x[:B], T, cond[:B]), off.drift_div(x[:B], T, cond[:B])
            assert on.debug_update_keep() == KEPT[F] and off.debug_update_keep() == 0
            assert np.isfinite(d0).all() and b1.tobytes() == b0.tobytes() and d1.tobytes() == d0.tobytes()
    finally:
        on.close(); off.close()


@pytest.mark.parametrize("F,L", [(32, 2), (128, 5)])
def test_six_molecules_against_the_fp64_oracle(monkeypatch, F, L):
    B = 6
    src, dst, et, flat, x, cond = model(F, L)
    grid = pkg().engine.time_grid(0.0, 1.0, 4)
    orc = oracle.PainnOracle(0, F, L, A, src, dst, et, np.arange(A), flat, temp_length=100.0)
    eng = engine(monkeypatch, F, L, True)
    try:
        eng.set_template("pair")
        got = eng.drift(x[:B], T, cond[:B])
        path, nfe = eng.rollout(x[:B], cond[:B], grid, scheme="em", eps=0.01, seed=7)
        assert eng.debug_update_keep() == KEPT[F] and nfe == 3
        ref = orc.drift(x[:B], T, cond[:B], precision=64)
        rp, _ = orc.rollout(x[:B], cond[:B], grid, scheme="em", eps=0.01, seed=7, precision=64)
        err, rerr = rel_l2(got, ref), rel_l2(path - path[0], rp - rp[0])
        print(f"F {F} L {L}: drift rel-L2 {err:.2e}, EM rollout rel-L2 {rerr:.2e}")
        assert err < DRIFT_TOL, err
        assert rerr < ROLLOUT_TOL, rerr
    finally:
        eng.close()
