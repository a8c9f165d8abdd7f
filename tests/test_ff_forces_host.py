"""Force-field forces and Langevin dynamics on the host: the numpy restatement (tests/ff_forces_numpy.py) against central differences
of the pinned energy and against itself in np.longdouble on the fixtures the GPU tests compare on, the integrator's restatement
(energy conservation, chaining, the noise keys, its own fp64 error d64), the dense tables of tests/ff_dense_numpy.py (their shape facts,
their conditioning, the runs beyond 64 components), the masses and constraints of the XML reader, and
drivers.generate_md against a stub engine.  No GPU."""
import functools
import os
import types

import numpy as np
import pytest

from conftest import GOLDEN, pkg
import ff_numpy as fn
import ff_forces_numpy as ffn
import ff_dense_numpy as fd
from test_forcefield import gpu_fixtures

XML = os.path.join(GOLDEN, "ff_small.xml")
LD = np.longdouble
wide = pytest.mark.skipif(np.finfo(LD).eps >= np.finfo(np.float64).eps, reason="np.longdouble is no wider than float64 here")


@functools.lru_cache(maxsize=None)
def fixtures():
    return gpu_fixtures()


# ---- 1. the restated forces ----------------------------------------------------------------------------------------------------
@wide
def test_analytic_forces_are_the_gradient_of_the_pinned_energy():
    """Central differences of the pinned energy (fn's term energies at 80-bit positions: ffn.energy_nm, checked here to be fn.energies
    bit for bit) against the restated forces, both in np.longdouble, as max |F - FD| / S^F over all components.  Measured (x86-64,
    80-bit long double), h = 1e-6 nm: A2 3.3e-9, A4 4.8e-9, A9 3.0e-9, A25 8.1e-8; h = 1e-7 nm: A2 3.3e-11, A4 4.8e-11, A9 1.9e-10,
    A25 8.1e-10 -- the h^2 truncation error of the difference quotient (the A25 geometries have close non-bonded contacts, so large
    third derivatives).  Bars: ten times the largest, 8.1e-7 and 8.1e-9, far below the 1e-4 a dropped or mis-signed term needs."""
    bars = {1e-6: 8.1e-7, 1e-7: 8.1e-9}
    assert max(bars.values()) < 1e-4
    for name, ff, x, to_nm in fixtures():
        A = x.shape[1]
        pairs = fn.pair_table(ff, A)
        p = x.astype(LD) * LD(np.float64(to_nm))
        F, S, E, _ = ffn.forces_nm(p, ff, pairs)
        E_pinned = fn.energies(x, to_nm, ff, ft=LD)[0]
        assert np.array_equal(ffn.energy_nm(p, ff, pairs), E_pinned) and np.array_equal(E, E_pinned), name
        for h, bar in bars.items():
            G = np.zeros_like(F)
            for a in range(A):
                for c in range(3):
                    up, dn = p.copy(), p.copy()
                    up[:, a, c] += LD(h); dn[:, a, c] -= LD(h)
                    G[:, a, c] = -(ffn.energy_nm(up, ff, pairs) - ffn.energy_nm(dn, ff, pairs)) / (2 * LD(h))
            r = float((np.abs(F - G) / S[..., None]).max())
            print(f"{name} h = {h:g}: max |F - FD| / S^F = {r:.2e} (bar {bar:.1e})")
            assert r <= bar, (name, h, r)


@wide
def test_the_restated_forces_are_well_conditioned():
    """|F64 - F80| <= 1e-13 S^F on every fixture, with and without T (measured: at most 4.6e-14), and the energy of the same pass
    without T is fn.energies bit for bit in both float types"""
    T = np.where(np.arange(67) % 2, 1000.0, 300.0).astype(np.float32)
    worst = 0.0
    for name, ff, x, to_nm in fixtures():
        for temps in (None, T):
            F64, S, E64 = ffn.forces(x, to_nm, ff, T=temps)
            F80, _, E80 = ffn.forces(x, to_nm, ff, T=temps, ft=LD)
            assert np.isfinite(F64).all()
            if temps is None:                                 # (with T, fn.energies divides the four sums, ffn.forces their total)
                assert np.array_equal(E64, fn.energies(x, to_nm, ff)[0]) and np.array_equal(E80, fn.energies(x, to_nm, ff, ft=LD)[0])
            r = float((np.abs((F64 - F80).astype(np.float64)) / S[..., None]).max())
            worst = max(worst, r)
            assert r <= 1e-13, (name, r)
    print(f"fp64 against 80-bit: worst |dF| / S^F = {worst:.2e}")


def test_known_forces():
    k, r0, r = 1000.0, 0.125, 0.25                            # exact in fp32 and fp64
    ff = dict(bond_idx=[[0, 1]], bond_par=[[r0, k]], angle_idx=np.zeros((0, 3)), angle_par=np.zeros((0, 2)), torsion_idx=np.zeros((0, 4)),
              torsion_par=np.zeros((0, 3)), particles=np.zeros((2, 3)), exceptions=np.zeros((0, 5)), coulomb=fn.COULOMB)
    F, S, E = ffn.forces(np.array([[[0, 0, 0], [r, 0, 0]]], np.float32), 1.0, ff)
    assert F[0].tolist() == [[k * (r - r0), 0, 0], [-k * (r - r0), 0, 0]] and S[0].tolist() == [1 + 125.0, 1 + 125.0] and E[0] == k * (r - r0) ** 2 / 2
    unit = dict(ff, bond_idx=np.zeros((0, 2)), bond_par=np.zeros((0, 2)), particles=[[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    F, _, _ = ffn.forces(np.array([[[0, 0, 0], [0.5, 0, 0]]], np.float32), 1.0, unit)
    assert F[0, 0, 0] == -fn.COULOMB / 0.25 and F[0, 1, 0] == fn.COULOMB / 0.25              # like charges repel
    F, _, E = ffn.forces(np.zeros((1, 2, 3), np.float32), 1.0, unit)                         # r = 0
    assert not np.isfinite(F).any()


# ---- 2. the restated integrator (A4, B = 3, 16 steps) -------------------------------------------------------------------------------
def md_case(name="A4", B=3):
    ff, x, to_nm = next((ff, x, to_nm) for n, ff, x, to_nm in fixtures() if n == name)
    pos = x[:B].astype(np.float64) * to_nm
    T = np.where(np.arange(B) % 2, 1000.0, 300.0).astype(np.float32)
    ids = np.arange(B, dtype=np.int64) + 7
    return ff, ffn.masses_for(ff), pos, T, ids, to_nm


def numpy_normal(seed, traj, step, comp):
    """a stand-in stream for the checks that do not concern the key: deterministic in its four arguments"""
    return np.float32(np.random.RandomState([seed % (1 << 32), traj % (1 << 32), step % (1 << 32), comp]).standard_normal())


def test_md_without_friction_conserves_the_energy_to_the_leapfrog_fluctuation():
    """With a = 1 the scheme is leapfrog with the stored velocity half a step behind the positions.  For a harmonic mode of frequency
    w it conserves m v_(n+1/2)^2 / 2 + k x_n x_(n+1) / 2 exactly, so the stored epot + ekin moves by k x_(n+1) (x_(n+1) - x_n) / 2: at
    most (w dt / 2) 2 E_mode, first order in dt.  Checked as: the largest excursion is within w_max dt times the largest kinetic energy
    plus potential excursion seen, w_max from the stiffest bond and its reduced mass; and halving dt halves it (between 1.5 and 3)."""
    ff, m, pos, T, ids, to_nm = md_case()
    vel = ffn.draw_velocities(T, ids, m, 3, 0, numpy_normal)
    bi, bp = np.asarray(ff["bond_idx"]), np.asarray(ff["bond_par"])
    w_max = np.sqrt(bp[:, 1] * (1.0 / m[bi[:, 0]] + 1.0 / m[bi[:, 1]])).max()                 # 1 / ps
    fluct = {}
    for dt, n in ((2.5e-4, 16), (1.25e-4, 32)):
        _, _, _, epot, ekin = ffn.langevin(pos, vel, T, ids, ff, m, dt, 0.0, n, stride=1, to_nm=to_nm, normal=None)
        tot = epot + ekin
        fluct[dt] = np.abs(tot - tot[:, :1]).max(axis=1)
        scale = w_max * dt * (ekin.max(axis=1) + (epot.max(axis=1) - epot.min(axis=1)))
        print(f"dt = {dt}: fluctuation {fluct[dt]}, bound {scale}")
        assert (fluct[dt] <= scale).all() and (fluct[dt] > 0).all()
    ratio = fluct[2.5e-4] / fluct[1.25e-4]
    assert ((ratio > 1.5) & (ratio < 3.0)).all(), ratio


def test_md_chained_equals_single_and_the_noise_is_the_oracles():
    from oracle import oracle
    ff, m, pos, T, ids, to_nm = md_case()
    kw = dict(ff=ff, masses=m, dt=5e-4, friction=1.0, seed=11, to_nm=to_nm)
    p16, v16, f16, e16, k16 = ffn.langevin(pos, None, T, ids, n_steps=16, stride=4, step_offset=5, draw=True, **kw)
    p8, v8, f8a, e8a, k8a = ffn.langevin(pos, None, T, ids, n_steps=8, stride=4, step_offset=5, draw=True, **kw)
    p8, v8, f8b, e8b, k8b = ffn.langevin(p8, v8, T, ids, n_steps=8, stride=4, step_offset=13, **kw)
    assert np.array_equal(p16, p8) and np.array_equal(v16, v8)
    assert np.array_equal(f16, np.concatenate([f8a, f8b], axis=1)) and np.array_equal(e16, np.concatenate([e8a, e8b], axis=1))
    assert np.array_equal(k16, np.concatenate([k8a, k8b], axis=1)) and f16.shape == (3, 4, 4, 3) and f16.dtype == np.float32
    assert np.abs(f16.astype(np.float64).mean(axis=2)).max() < 1e-6                            # centred to fp32 round-off
    # one step from rest at friction so large that a = 0: v = sqrt(R T / m) xi, so xi is read back and must be oracle.normal at
    # (seed, id, step_offset + s, 3a + c)
    A = 4
    far = dict(kw, friction=1e6)
    _, v1, _, _, _ = ffn.langevin(pos, np.zeros_like(pos), T, ids, n_steps=1, step_offset=41, **far)
    amp = np.sqrt(fn.R_GAS * T.astype(np.float64)[:, None] / m[None, :])[..., None]
    want = np.array([[oracle.normal(11, int(i), 41, c) for c in range(3 * A)] for i in ids], np.float32).reshape(3, A, 3)
    np.testing.assert_allclose(v1 / amp, want.astype(np.float64), rtol=1e-14, atol=0)
    v0 = ffn.draw_velocities(T, ids, m, 11, 41)                                                 # components 3A .. 6A - 1 of the same step
    want0 = np.array([[oracle.normal(11, int(i), 41, 3 * A + c) for c in range(3 * A)] for i in ids], np.float32).reshape(3, A, 3)
    np.testing.assert_allclose(v0 / amp, want0.astype(np.float64), rtol=1e-14, atol=0)


@wide
def test_md_fp64_error_d64_is_recorded():
    """d64: the fp64 restatement against the same code in np.longdouble over the GPU trajectory test's run (A4 and A9, B = 5, 300 /
    1000 K, dt = 0.5 fs, friction = 1 / ps, 16 steps), as the largest |difference| of a position (nm) or velocity (nm / ps) component.
    tests/test_gpu_md.py computes it the same way (md_d64) and holds the GPU to 100 d64."""
    for name in ("A4", "A9"):
        d = md_d64(name)
        print(f"{name}: d64 = {d:.3e}")
        assert 0 < d < 1e-9                                   # fp64 round-off over 16 steps, not a divergence


def md_d64(name):
    ff, m, pos, T, ids, to_nm = md_case(name, 5)
    kw = dict(ff=ff, masses=m, dt=5e-4, friction=1.0, n_steps=16, stride=4, seed=11, to_nm=to_nm, draw=True)
    p64, v64, _, _, _ = ffn.langevin(pos, None, T, ids, **kw)
    p80, v80, _, _, _ = ffn.langevin(pos, None, T, ids, ft=LD, **kw)
    return float(max(np.abs(p64 - p80).max(), np.abs(v64 - v80).max()))


# ---- 2b. the dense tables and the runs beyond 64 components (tests/test_gpu_ff_edges.py, tests/test_gpu_md_edges.py) -----------------
def test_the_dense_cases_sit_on_their_edges():
    """the shape facts each case of ff_dense_numpy.CASES exists for, so that an edit of the builder cannot move one off its edge"""
    chunks = lambda n: (n + 63) // 64
    for name, (A, nb, na, nt, hub) in fd.CASES.items():
        ff, x, to_nm = fd.dense_case(name)
        assert x.shape == (fd.B_DENSE, A, 3) and x.dtype == np.float32 and fd.B_DENSE == 9, name
        assert [len(ff[k]) for k in ("bond_idx", "angle_idx", "torsion_idx")] == [nb, na, nt], name
        assert len(ff["bond_par"]) == nb and len(ff["angle_par"]) == na and ff["torsion_par"].shape == (nt, 3), name
        for key, slots in (("bond_idx", 2), ("angle_idx", 3), ("torsion_idx", 4)):                 # what ti_obs_ff_set accepts
            idx = np.asarray(ff[key])
            assert idx.shape == (len(idx), slots) and (idx >= 0).all() and (idx < A).all(), (name, key)
            assert all(len(set(row)) == slots for row in idx.tolist()), (name, key)
        assert set(ff["torsion_par"][:, 0].tolist()) <= {1.0, 2.0, 3.0, 4.0, 5.0, 6.0} and set(ff["torsion_par"][:, 1].tolist()) <= {0.0, np.pi}, name
        inc = fd.incidence(ff, A)
        assert inc.shape == (chunks(nb) + chunks(na) + chunks(nt), A) and inc.sum() == 2 * nb + 3 * na + 4 * nt, name
        again = fd.dense_forcefield(A, nb, na, nt, fd.B_DENSE, seed=0, hub=hub)                    # deterministic
        assert all(np.array_equal(ff[k], again[0][k]) for k in ff if k != "coulomb") and np.array_equal(x, again[1]), name
    counts = {name: (c[0], tuple(c[1:4])) for name, c in fd.CASES.items()}
    assert counts["all_caps"] == (25, (64, 128, 512)) and fd.incidence(fd.dense_case("all_caps")[0], 25).shape[0] == 11
    assert fd.incidence(fd.dense_case("all_caps")[0], 25).sum() == 2560                           # the incidence bytes at their cap
    assert counts["angles_2nd"] == (25, (24, 65, 64)) and counts["no_bonds"] == (25, (0, 65, 65)) and counts["tors_only"] == (25, (0, 0, 129))
    assert counts["pairs_only"] == (24, (0, 0, 0)) and fd.incidence(fd.dense_case("pairs_only")[0], 24).shape == (0, 24)
    assert fn.pair_table(fd.dense_case("pairs_only")[0], 24)[:, [0, 2]].any()                      # and live pairs
    assert counts["below_half"] == (21, (63, 128, 129)) and 3 * 21 == 63 and (21 + 1) // 2 % 2 == 1
    assert counts["three_atoms"] == (3, (2, 3, 0)) and (3 + 1) // 2 == 2
    assert counts["hub"] == (22, (64, 64, 65)) and fd.CASES["hub"][4] and 3 * 22 == 66
    ff = fd.dense_case("hub")[0]
    inc = fd.incidence(ff, 22)
    assert (ff["bond_idx"][:, 0] == 0).all() and inc[0, 0] == 64 and inc[0].sum() == 128          # atom 0 in all 64 terms of chunk 0
    assert (inc[0, 12:] == 0).all() and (inc[0] == 0).sum() >= 10                                  # and atoms with no entry in it
    for name in ("all_caps", "angles_2nd", "no_bonds", "tors_only"):                              # both components of a lane
        assert 3 * fd.CASES[name][0] > 64


@wide
def test_the_dense_cases_are_well_conditioned():
    """The restatement on the dense tables against itself in np.longdouble: |F64 - F80| <= 1e-13 S^F and |E64 - E80| <= 1e-13 S_b, the
    bars of the tree fixtures, with and without T (measured: 2.8e-15 and 1.9e-15 at worst)"""
    T = np.where(np.arange(fd.B_DENSE) % 2, 1000.0, 300.0).astype(np.float32)
    worst_f = worst_e = 0.0
    for name in fd.CASES:
        ff, x, to_nm = fd.dense_case(name)
        for temps in (None, T):
            F64, S, E64 = ffn.forces(x, to_nm, ff, T=temps)
            F80, _, E80 = ffn.forces(x, to_nm, ff, T=temps, ft=LD)
            E64n, s64, Sb, _ = fn.energies(x, to_nm, ff, T=temps)
            E80n, s80, _, _ = fn.energies(x, to_nm, ff, T=temps, ft=LD)
            Sb = Sb if temps is None else Sb / (fn.R_GAS * temps.astype(np.float64))[:, None]
            assert np.isfinite(F64).all() and np.isfinite(E64).all() and np.isfinite(E64n).all(), name
            rf = float((np.abs((F64 - F80).astype(np.float64)) / S[..., None]).max())
            re = float(max((np.abs((E64 - E80).astype(np.float64)) / Sb.sum(axis=1)).max(),
                           (np.abs((E64n - E80n).astype(np.float64)) / Sb.sum(axis=1)).max(),
                           (np.abs((s64 - s80).astype(np.float64)) / np.maximum(Sb, 1.0)).max()))
            worst_f, worst_e = max(worst_f, rf), max(worst_e, re)
            assert rf <= 1e-13 and re <= 1e-13, (name, rf, re)
    print(f"dense tables, fp64 against 80-bit: worst |dF| / S^F = {worst_f:.2e}, |dE| / S_b = {worst_e:.2e}")


BIG_IDS = np.array([7, 2 ** 32 + 1, 2 ** 40 + 9, 2 ** 62 + 3, -2], np.int64)
BIG_SEED = 2 ** 40 + 11
SMALL_DT = dict(dt=1e-5, friction=1.0, n_steps=16, stride=4, seed=11)


@functools.lru_cache(maxsize=None)
def md_edge_case(name):
    """(ff, masses, pos [5, A, 3] nm, T [5], ids [5], to_nm, run) of the integrator's runs beyond 64 components and with 64-bit keys:
    "A25" (the tree fixture, three torsion chunks), "hub" (A = 22, dense), "all_caps" (A = 25, every table at its cap, 4 steps) at
    dt = 0.01 fs -- the tree geometries carry Lennard-Jones contacts with forces of order 1e8 kJ / (mol nm), under which the
    restatement itself flies apart at the 0.5 fs of the A4 / A9 runs (A9 with these keys: a coordinate moves by 18 nm in 16 steps) --
    and "A9_ids": the A9 fixture at the same dt with replica ids and a seed beyond 32 bits."""
    B = 5
    T = np.where(np.arange(B) % 2, 1000.0, 300.0).astype(np.float32)
    ids = np.arange(B, dtype=np.int64) * 3 + 7
    run = dict(SMALL_DT)
    if name in ("A25", "A9_ids"):
        ff, x, to_nm = next((ff, x, to_nm) for n, ff, x, to_nm in fixtures() if n == name.split("_")[0])
        m = ffn.masses_for(ff)
        if name == "A9_ids":
            ids, run = BIG_IDS.copy(), dict(SMALL_DT, seed=BIG_SEED)
    else:
        ff, x, to_nm = fd.dense_case(name)
        m = np.full(x.shape[1], 12.0)
        if name == "all_caps":
            run.update(n_steps=4, stride=2)
    return ff, m, x[:B].astype(np.float64) * to_nm, T, ids, to_nm, run


def md_edge_d64(name):
    """(d64, the restatement's largest displacement of an atom's coordinate over the run, in nm)"""
    ff, m, pos, T, ids, to_nm, run = md_edge_case(name)
    kw = dict(ff=ff, masses=m, to_nm=to_nm, draw=True, **run)
    p64, v64, _, _, _ = ffn.langevin(pos, None, T, ids, **kw)
    p80, v80, _, _, _ = ffn.langevin(pos, None, T, ids, ft=LD, **kw)
    one = dict(kw, n_steps=1, stride=0, draw=False)
    p, v, moved = pos, ffn.draw_velocities(T, ids, m, run["seed"], 0), 0.0
    for s in range(run["n_steps"]):                            # the same run a step at a time (chaining repeats it bit for bit)
        p, v, _, _, _ = ffn.langevin(p, v, T, ids, step_offset=s, **one)
        moved = max(moved, float(np.abs(p - pos).max()))
    assert np.array_equal(p, p64) and np.array_equal(v, v64)
    return float(max(np.abs(p64 - p80).max(), np.abs(v64 - v80).max())), moved


@wide
def test_md_edge_runs_stay_bounded_and_conditioned():
    """What makes the GPU comparison of tests/test_gpu_md_edges.py meaningful: over each run the restatement moves no coordinate by more
    than 0.5 nm and its own fp64 error d64 is at most 1e-10.  Measured: A25 0.21 nm, d64 8.1e-13; hub 0.013 nm, 1.1e-13; all_caps
    0.012 nm, 2.3e-13; A9_ids 0.052 nm, 3.8e-13."""
    for name in ("A25", "hub", "all_caps", "A9_ids"):
        A = md_edge_case(name)[2].shape[1]
        assert 3 * A > 64 or name == "A9_ids", name               # components 64 .. 3A - 1, velocity draws up to 6A - 1
        d, moved = md_edge_d64(name)
        print(f"{name}: d64 = {d:.3e}, largest displacement {moved:.3e} nm")
        assert 0 < d <= 1e-10 and moved <= 0.5, (name, d, moved)
    assert 6 * 25 - 1 == 149


# ---- 3. the reader ----------------------------------------------------------------------------------------------------------------
def test_from_openmm_xml_reads_the_masses_and_records_constraints():
    ti = pkg()
    ff = ti.forcefield.ForceField.from_openmm_xml(XML)
    assert ff.masses.dtype == np.float64 and ff.masses.tolist() == [12.01, 12.01, 14.01, 15.999, 1.008] and ff.has_constraints is False
    text = open(XML).read()
    assert text.count("<Constraints/>") == 1
    held = ti.forcefield.ForceField.from_openmm_xml(text.replace("<Constraints/>", '<Constraints><Constraint d=".101" p1="2" p2="4"/></Constraints>'))
    assert held.has_constraints is True and held.masses.tolist() == ff.masses.tolist()
    np.testing.assert_array_equal(held.pair_table(), ff.pair_table())                          # the energies ignore them, as before
    assert ti.forcefield.ForceField(particles=np.zeros((3, 3))).masses is None
    with pytest.raises(ValueError, match="masses"):
        ti.forcefield.ForceField(particles=np.zeros((3, 3)), masses=[1.0, 2.0])


def test_langevin_refuses_constraints_and_missing_masses_before_the_library():
    """PainnEngine.langevin's own refusals need no device: an engine object without a handle stands in"""
    ti = pkg()
    eng = object.__new__(ti.engine.PainnEngine)
    eng.A = 5
    pos = np.zeros((2, 5, 3))
    with pytest.raises(ValueError, match="force field"):
        eng.langevin(pos, pos, 300.0, 1e-3, 1.0, 1)
    eng._ff_set, eng._ff_constraints, eng._ff_masses = True, True, True
    with pytest.raises(ValueError, match="constraints"):
        eng.langevin(pos, pos, 300.0, 1e-3, 1.0, 1)
    eng._ff_constraints, eng._ff_masses = False, False
    with pytest.raises(ValueError, match="masses"):
        eng.langevin(pos, pos, 300.0, 1e-3, 1.0, 1)


# ---- 4. the driver against a stub engine -------------------------------------------------------------------------------------------
class StubEngine:
    """What md.LangevinSampler asks of an engine; frames carry (replica id, frame number of the whole run) so the layout can be read"""

    def __init__(self):
        self.calls, self.ff = [], None

    def set_forcefield(self, ff):
        self.ff = ff

    def langevin(self, pos, vel, T, dt, friction, n_steps, stride=0, step_offset=0, seed=0, ids=None, to_nm=1.0, draw_velocities=False,
                 steps_per_launch=0, **kw):
        self.calls.append(dict(n_steps=n_steps, stride=stride, step_offset=step_offset, draw=draw_velocities, T=np.array(T), ids=np.array(ids),
                               dt=dt, friction=friction, seed=seed, to_nm=to_nm, pos=np.array(pos)))
        B, A = pos.shape[:2]
        nf = n_steps // stride if stride else 0
        frames = np.zeros((B, nf, A, 3), np.float32)
        frames[..., 0] = np.asarray(ids, np.float32)[:, None, None]
        frames[..., 1] = ((step_offset + stride * (1 + np.arange(nf))) if nf else np.zeros(0))[None, :, None]
        frames[..., 2] = np.asarray(T)[:, None, None]
        e = np.tile(np.asarray(ids, np.float64)[:, None], (1, nf))
        return np.array(pos), np.zeros_like(pos), (frames if nf else None), (e if nf else None), (e + 0.5 if nf else None)


def md_config(tmp_path, **over):
    x0 = np.arange(2 * 5 * 3, dtype=np.float64).reshape(2, 5, 3)
    np.save(tmp_path / "x0.npy", x0)
    cfg = dict(forcefield=XML, x0=str(tmp_path / "x0.npy"), scale=10.0, temperatures=[300, 1000], n_replicas=5, dt=1e-3, friction=1.0,
               n_equil=7, n_frames=3, stride=2, seed=9, splits={"train": 0.6, "val": 0.2, "test": 0.2}, traj_path=str(tmp_path / "out"),
               traj_filename="mol.npy")
    cfg.update(over)
    return types.SimpleNamespace(**cfg), x0


def test_generate_md_layout_splits_and_round_trip(tmp_path):
    ti = pkg()
    cfg, x0 = md_config(tmp_path)
    eng = StubEngine()
    paths = ti.drivers.generate_md(cfg, eng)
    assert sorted(paths) == ["test", "train", "val"] and eng.ff.n_atoms == 5
    draw, equil, run = eng.calls
    assert (draw["n_steps"], draw["draw"], draw["step_offset"]) == (0, True, 0) and draw["to_nm"] == 0.1
    assert (equil["n_steps"], equil["stride"], equil["step_offset"], equil["draw"]) == (7, 0, 0, False)
    assert (run["n_steps"], run["stride"], run["step_offset"]) == (6, 2, 7)                    # the step index runs on
    assert run["T"].tolist() == [300.0] * 5 + [1000.0] * 5 and run["ids"].tolist() == list(range(10)) and run["seed"] == 9
    np.testing.assert_array_equal(draw["pos"], x0[np.arange(10) % 2] * 0.1)                     # the geometries in turn, in nm
    first = 0
    for split, n in (("train", 3), ("val", 1), ("test", 1)):                                    # whole replicas, in the order of the key
        a = np.load(paths[split])
        assert a.dtype == np.float32 and a.shape == (8, n * 3, 5, 3) and paths[split] == os.path.join(cfg.traj_path, split, "mol.npy")
        assert np.isnan(a[1:7]).all() and np.isfinite(a[[0, 7]]).all()                          # 400 .. 900 K were not simulated
        for row, k in ((0, 0), (7, 1)):
            want_ids = np.repeat(k * 5 + first + np.arange(n), 3)                               # replica-major
            np.testing.assert_array_equal(a[row, :, 0, 0], want_ids)
            np.testing.assert_array_equal(a[row, :, 0, 1], np.tile([9, 11, 13], n))             # frames after steps 9, 11, 13 of the run
            assert (a[row, :, 0, 2] == (300.0, 1000.0)[k]).all()
        first += n
        got = ti.data.load_trajectory(cfg.traj_path, split, "mol.npy", 1000, scale=False)       # the loader's view: centred again
        assert got.shape == (n * 3, 5, 3) and got.dtype == np.float32
        np.testing.assert_allclose(got, a[7] - a[7].mean(axis=1, keepdims=True), atol=1e-6)
    with np.load(os.path.join(cfg.traj_path, "md_log.npz")) as z:
        assert z["epot"].shape == z["ekin"].shape == (2, 5, 3) and int(z["seed"]) == 9 and int(z["n_equil"]) == 7 and float(z["to_nm"]) == 0.1
        assert z["temperatures"].tolist() == [300, 1000] and z["split_names"].tolist() == ["train", "val", "test"] and z["split_replicas"].tolist() == [3, 1, 1]
        np.testing.assert_array_equal(z["epot"][1, :, 0], 5 + np.arange(5))


@pytest.mark.parametrize("over,named", [(dict(temperatures=[300, 350]), "temperatures"), (dict(temperatures=[300, 300]), "temperatures"),
                                        (dict(to_nm=0.1), "exactly one"), (dict(scale=None), "exactly one"), (dict(scale=0.0), "finite"),
                                        (dict(splits={"train": 0.9, "val": 0.05}), "without a replica"), (dict(splits={"a": 0.7, "b": 0.7}), "splits"),
                                        (dict(n_frames=0), "n_frames"), (dict(seed=None), "seed")])
def test_generate_md_checks_its_keys_before_it_runs(tmp_path, over, named):
    ti = pkg()
    cfg, _ = md_config(tmp_path, **over)
    eng = StubEngine()
    with pytest.raises(ValueError, match=named):
        ti.drivers.generate_md(cfg, eng)
    assert not eng.calls and not os.path.exists(cfg.traj_path)
