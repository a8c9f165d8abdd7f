"""The optimiser shell the adw and the cPaiNN trainer share (csrc/train_optim.hpp, engine._Trainer), on both: a many-step call from
host memory against the same call from device memory, out-of-range indices into either set in either memory space, state moved into
a trainer of other weights, set_lr against a trainer created with that rate.  Every assertion is on bits.

Shapes: adw H = 32, L = 1, d = 2, sets of 8 rows, B = 4, 3 steps; cPaiNN single-T and ambient at F = 32, L = 1, A = 3 with all six
directed edges, sets of 4, B = 2, 3 steps -- more than one step, gathers that are not the identity.

Left to the tests that already assert them for both trainers: apply(grad()["grad"]) against a step on the same batch
(test_gpu_adw_train.test_steps_compose_bit_for_bit, test_gpu_painn_train.test_step_is_grad_then_apply)."""
import numpy as np
import pytest
import torch

import adw_train_numpy as an
import painn_train_cases as pc
from conftest import pkg

pytestmark = pytest.mark.gpu
STEPS = 3
KEYS = ("w", "m", "v", "n_applied", "n_skipped")


class Adw:
    H, L, d, n, B = 32, 1, 2, 8, 4

    def __init__(self):
        rs = np.random.RandomState(3)
        self.sets = [rs.standard_normal((self.n, self.d)).astype(np.float32), (1.0 + rs.standard_normal((self.n, self.d))).astype(np.float32),
                     rs.choice([0.5, 1.0], self.n).astype(np.float32), rs.choice([1.25, 1.5], self.n).astype(np.float32)]
        self.kw = dict(kind="standard", a=0.9, seed=5)

    def trainer(self, seed=0, **kw):
        sd = pkg().synthetic.make_state_dict(an.spec(self.H, self.L, self.d), seed, np.float64)
        return pkg().engine.AdwTrainer(self.H, self.L, an.flat(sd, self.H, self.L, self.d), dim=self.d, weight_decay=1e-5, **kw)

    def steps(self, tr, i0, i1, to=lambda v: v, draw=0):
        return tr.steps(*(to(v) for v in self.sets), to(i0), to(i1), draw=draw, **self.kw)


class Painn:
    F, L, A, n, B = 32, 1, 3, 4, 2

    def __init__(self, variant, kind):
        self.variant = variant
        self.c = pc.make_case(variant, self.F, self.L, self.A, self.n, tpl="full", kind=kind, seed=2)
        ncond = {0: 2, 1: 1, 2: 0}[variant]
        temps = [(300.0 + 100.0 * (np.arange(self.n) % 3)).astype(np.float32), (400.0 + 100.0 * (np.arange(self.n) % 4)).astype(np.float32)]
        self.sets = [self.c["x0"], self.c["x1"], temps[0] if ncond == 2 else None, temps[1] if ncond >= 1 else None]
        self.kw = dict(kind=kind, seed=77, traj_offset=9)

    def trainer(self, seed=2, **kw):
        c = self.c if seed == 2 else pc.make_case(self.variant, self.F, self.L, self.A, self.n, tpl="full", seed=seed)
        return pc.make_trainer(c, weight_decay=1e-5, **kw)

    def steps(self, tr, i0, i1, to=lambda v: v, draw=0):
        x0, x1, t0, t1 = (None if v is None else to(v) for v in self.sets)
        return tr.steps(x0, x1, t0, t1, to(i0), to(i1), draw=draw, **self.kw)


CASES = {"adw": Adw, "painn-single-T": lambda: Painn(2, "one_sided"), "painn-ambient": lambda: Painn(0, "standard")}


@pytest.fixture(params=list(CASES))
def case(request):
    return CASES[request.param]()


def _idx(c, seed=1):
    rs = np.random.RandomState(seed)
    return rs.randint(0, c.n, (STEPS, c.B)).astype(np.int64), rs.randint(0, c.n, (STEPS, c.B)).astype(np.int64)


def _dev(v):
    return torch.from_numpy(np.ascontiguousarray(v)).cuda()


def _same(a, b):
    sa, sb = (a if isinstance(a, dict) else a.state()), (b if isinstance(b, dict) else b.state())
    return all(np.array_equal(sa[k], sb[k]) for k in KEYS)


def test_host_and_device_calls_give_the_same_bits(case):
    i0, i1 = _idx(case)
    th, td = case.trainer(), case.trainer()
    lh, sh = case.steps(th, i0, i1)
    ld, sd = case.steps(td, i0, i1, to=_dev)
    assert sh == sd == 0 and np.array_equal(lh, ld) and np.all(np.isfinite(lh)) and _same(th, td)
    assert th.state()["n_applied"] == STEPS


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("to", [lambda v: v, _dev], ids=["host", "device"])
def test_an_index_past_a_set_is_refused_and_leaves_no_trace(case, to, which):
    i0, i1 = _idx(case)
    tr, fresh = case.trainer(), case.trainer()
    before = tr.state()
    bad = [i0.copy(), i1.copy()]
    bad[which][1, 1] = case.n                   # n0 == n1 == n: the first index past the set
    with pytest.raises(pkg()._lib.TiError, match=rf"idx{which}\[{case.B + 1}\]") as e:
        case.steps(tr, bad[0], bad[1], to=to)
    assert e.value.code == pkg()._lib.TI_E_ARG and _same(before, tr)
    la, _ = case.steps(tr, i0, i1, to=to)
    lb, _ = case.steps(fresh, i0, i1, to=to)
    assert np.array_equal(la, lb) and _same(tr, fresh)


def test_state_moves_into_a_trainer_of_other_weights(case):
    i0, i1 = _idx(case)
    j0, j1 = _idx(case, seed=2)
    a, b = case.trainer(), case.trainer(seed=11)
    assert not np.array_equal(a.weights(), b.weights())
    case.steps(a, i0, i1)
    b.load_state(**a.state())
    assert _same(a, b)
    la, _ = case.steps(a, j0, j1, draw=STEPS)
    lb, _ = case.steps(b, j0, j1, draw=STEPS)
    assert np.array_equal(la, lb) and _same(a, b) and a.state()["n_applied"] == 2 * STEPS


def test_set_lr_is_a_trainer_created_with_that_rate(case):
    i0, i1 = _idx(case)
    a, b = case.trainer(lr=1e-3), case.trainer(lr=2.5e-4)
    case.steps(a, i0, i1)
    b.load_state(**a.state())
    a.set_lr(2.5e-4)
    la, _ = case.steps(a, i0[:1], i1[:1], draw=STEPS)
    lb, _ = case.steps(b, i0[:1], i1[:1], draw=STEPS)
    assert np.array_equal(la, lb) and _same(a, b) and a.state()["n_applied"] == STEPS + 1
