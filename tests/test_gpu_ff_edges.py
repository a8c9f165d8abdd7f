"""ti_obs_ff_forces and ti_obs_ff_energy at the table and size edges the tree fixtures do not reach, against the numpy restatements
(tests/ff_forces_numpy.py, tests/ff_numpy.py) on the dense tables of tests/ff_dense_numpy.py: a second angle chunk, empty tables in
front of full ones, every table at its cap (11 chunks, 2560 incidence bytes), one atom in all 64 terms of a chunk, 3A = 63 and 66,
three atoms, no bonded term at all; the torsion chunk edges 64 / 65 of the tree through the forces; and a batch of 16389 molecules,
whose last five take the grid-stride loop's second trip.  Bars and contract: those of tests/test_gpu_ff_forces.py and
tests/test_gpu_forcefield.py, through their own checks; tests/test_ff_forces_host.py holds the restatement on these tables to 1e-13.

Largest |GPU - numpy| / S^F per case, MI355X: profiles/ff_forces_parity.txt."""
import functools

import numpy as np
import pytest

from conftest import pkg
import ff_numpy as fn
import ff_forces_numpy as ffn
import ff_dense_numpy as fd
import test_gpu_forcefield as tge
import test_gpu_ff_forces as tgf
from test_gpu_forcefield import engine, bits

pytestmark = pytest.mark.gpu

BATCHES = (1, 5, fd.B_DENSE)
ALONE = (0, 3, 4, 8)              # the first and the last wave of a workgroup, the first of the next, the last molecule


def references(ff, x, to_nm, T):
    """((F, S^F, E, S_b) without T, with T), ((E, sums, S) without T, with T): what check_forces and check_energies compare with"""
    f_refs, e_refs = [], []
    for temps in (None, T):
        F, S, E = ffn.forces(x, to_nm, ff, T=temps)
        En, sums, Scol, _ = fn.energies(x, to_nm, ff, T=temps)
        Scol = Scol if temps is None else Scol / (fn.R_GAS * temps.astype(np.float64))[:, None]
        f_refs.append((F, S, E, Scol.sum(axis=1)))
        e_refs.append((En, sums, Scol))
    return f_refs, e_refs


@functools.lru_cache(maxsize=None)
def dense(name):
    ff, x, to_nm = fd.dense_case(name)
    T = np.where(np.arange(len(x)) % 2, 1000.0, 300.0).astype(np.float32)
    return (ff, x, to_nm, T) + references(ff, x, to_nm, T)


def loaded(ff, A):
    """the shared handle for A atoms with ff in force -- for A = 3 a handle of its own: tests/test_gpu_forcefield.py's refusals need the
    shared one as a handle that never had a force field"""
    eng = engine.__wrapped__(A) if A == 3 else engine(A)
    eng.set_forcefield(pkg().forcefield.ForceField(**ff))
    return eng


@pytest.mark.parametrize("name", list(fd.CASES))
def test_dense_tables_forces_and_energies(name):
    pytest.importorskip("torch")
    ff, x, to_nm, T, f_refs, e_refs = dense(name)
    eng = loaded(ff, x.shape[1])
    tgf.check_forces(name, eng, ff, x, to_nm, T, f_refs[0], f_refs[1], batches=BATCHES, alone=ALONE)
    tge.check_energies(name, eng, x, to_nm, T, e_refs[0], e_refs[1], batches=BATCHES, alone=ALONE)


@pytest.mark.parametrize("name", ["A25_t64", "A25_t65"])
def test_tree_torsion_chunk_edges_through_the_forces(name):
    """the tree of 25 atoms with its torsion table cut to exactly one chunk and to one term more: pinned for the energy kernel in
    tests/test_gpu_forcefield.py, here for the forces, the only reader of the incidence list"""
    pytest.importorskip("torch")
    ff, x, to_nm, T, _, _ = tge.cases()[name]
    assert len(ff["torsion_idx"]) == int(name[-2:])
    f_refs, _ = references(ff, x, to_nm, T)
    tgf.check_forces(name, loaded(ff, 25), ff, x, to_nm, T, f_refs[0], f_refs[1])


# ---- the second trip of the grid-stride loop ------------------------------------------------------------------------------------------
GROUPS, WAVES = 4096, 4           # launch_obs_ff_forces: at most 4096 workgroups of four waves, one molecule a wave
B_TRIP = GROUPS * WAVES + 5       # 16389: workgroup 0 comes round again with all four waves, workgroup 1 with one, three idle


@functools.lru_cache(maxsize=None)
def second_trip():
    """the A4 fixture's force field and 16389 distinct molecules: the 67 fixture molecules in turn, copy b scaled by 1 + b 2^-21 (at
    most 0.8 %, exact in fp32 before the product is rounded)"""
    ff, x67, to_nm = next((ff, x, to_nm) for n, ff, x, to_nm in tge.gpu_fixtures() if n == "A4")
    b = np.arange(B_TRIP)
    x = (x67[b % 67] * (np.float32(1) + b.astype(np.float32) * np.float32(2.0 ** -21))[:, None, None]).astype(np.float32)
    assert len(np.unique(x.reshape(B_TRIP, -1), axis=0)) == B_TRIP
    T = np.where(b % 2, 1000.0, 300.0).astype(np.float32)
    return (ff, x, to_nm, T) + references(ff, x, to_nm, T)


def test_second_trip_of_the_grid_stride_loop():
    ti = pkg()
    ff, x, to_nm, T, f_refs, e_refs = second_trip()
    eng = loaded(ff, 4)
    assert B_TRIP == 16389 and B_TRIP > GROUPS * WAVES
    cut = GROUPS * WAVES
    for temps, fref, eref in ((None, f_refs[0], e_refs[0]), (T, f_refs[1], e_refs[1])):
        F, S, E, Sb = fref
        f, e = eng.ff_forces(x, to_nm, temps, energy=True)
        rf, re = float((np.abs(f - F) / S[..., None]).max()), float((np.abs(e - E) / Sb).max())
        tail = float((np.abs(f[cut:] - F[cut:]) / S[cut:, :, None]).max())
        print(f"second trip T={'yes' if temps is not None else 'no'}: |dF| / S^F = {rf:.3e} (molecules 16384 .. 16388: {tail:.3e}), |dE| / S_b = {re:.3e}")
        assert np.isfinite(f).all() and np.isfinite(e).all()
        assert (np.abs(f - F) <= tgf.TOL * S[..., None]).all(), rf
        assert (np.abs(e - E) <= tgf.TOL * Sb).all(), re
        en, terms = eng.ff_energy(x, to_nm, temps, terms=True)
        tge.check("second_trip", en, terms, eref, B_TRIP)
        # the batch does not enter: the same molecules in calls of at most 16384 (one trip each) give the same bits
        sl = lambda a, lo, hi: None if a is None else a[lo:hi]
        for lo, hi in ((0, cut), (cut, B_TRIP), (cut - 3, B_TRIP), (B_TRIP - 1, B_TRIP)):
            fp, ep = eng.ff_forces(x[lo:hi], to_nm, sl(temps, lo, hi), energy=True)
            np.testing.assert_array_equal(bits(fp), bits(f[lo:hi])); np.testing.assert_array_equal(bits(ep), bits(e[lo:hi]))
            enp, tp = eng.ff_energy(x[lo:hi], to_nm, sl(temps, lo, hi), terms=True)
            np.testing.assert_array_equal(bits(enp), bits(en[lo:hi])); np.testing.assert_array_equal(bits(tp), bits(terms[lo:hi]))
        np.testing.assert_array_equal(bits(eng.ff_forces(x, to_nm, temps)), bits(f))               # energy off; and the same call twice
    # a bad temperature in the second trip and an earlier one in the first: the first is named, nothing is written
    Tb = T.copy()
    Tb[16388], Tb[9000] = 0.0, np.nan
    rc, f, e = tgf.raw_forces(eng.h, x, Tb)
    assert rc == ti._lib.TI_E_ARG and "index 9000" in ti._lib.last_error() and (f == -7.0).all() and (e == -7.0).all()
    rc, e, terms = tge.raw_energy(eng.h, x, Tb)
    assert rc == ti._lib.TI_E_ARG and "index 9000" in ti._lib.last_error() and (e == -7.0).all() and (terms == -7.0).all()
    Tb[9000] = 300.0
    rc, f, e = tgf.raw_forces(eng.h, x, Tb)
    assert rc == ti._lib.TI_E_ARG and "index 16388" in ti._lib.last_error() and (f == -7.0).all() and (e == -7.0).all()
