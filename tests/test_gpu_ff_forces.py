"""ti_obs_ff_forces on the GPU against the numpy restatement (tests/ff_forces_numpy.py): every component within 1e-11 S^F of its atom
(S^F[b, a] = 1 + the sum over the terms touching atom a of the norm of their contribution; tests/test_ff_forces_host.py holds the
restatement to 1e-13 S^F against 80-bit arithmetic and to central differences of the pinned energy on the same fixtures), the energy of
the same pass within the energy tests' 1e-11 S_b, the reduced values with T, zero net force and torque, the bitwise contract (repeat,
alone, reversed, host against device memory), poisoned molecules and the refusals with their outputs untouched.

Largest |GPU - numpy| / S^F per case, MI355X: profiles/ff_forces_parity.txt."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from conftest import pkg
import ff_numpy as fn
import ff_forces_numpy as ffn
from test_forcefield import gpu_fixtures
from test_gpu_forcefield import engine, bits

pytestmark = pytest.mark.gpu

TOL = 1e-11
B_FULL = 67
BATCHES = (1, 5, B_FULL)          # one molecule; fewer than a workgroup's four; not a multiple of four


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (force field dict, x [67, A, 3], to_nm, T [67], (F, S^F, E, S_b) without T, the same with T); computed once"""
    T = np.where(np.arange(B_FULL) % 2, 1000.0, 300.0).astype(np.float32)
    out = {}
    for name, ff, x, to_nm in gpu_fixtures():
        refs = []
        for temps in (None, T):
            F, S, E = ffn.forces(x, to_nm, ff, T=temps)
            Sb = fn.energies(x, to_nm, ff, T=temps)[2].sum(axis=1)
            Sb = Sb if temps is None else Sb / (fn.R_GAS * temps.astype(np.float64))
            refs.append((F, S, E, Sb))
        out[name] = (ff, x, to_nm, T, refs[0], refs[1])
    return out


def with_ff(name):
    ti = pkg()
    ff, x, to_nm, T, r0, r1 = cases()[name]
    eng = engine(x.shape[1])
    eng.set_forcefield(ti.forcefield.ForceField(**ff))
    return eng, x, to_nm, T, r0, r1


def check_forces(name, eng, ff, x, to_nm, T, ref0, ref1, batches=BATCHES, alone=(0, 3, 4, 65, 66)):
    """The parity and the bitwise contract of ti_obs_ff_forces for one species: x [n, A, 3] with n = the largest of `batches`, the
    references (F, S^F, E, S_b) without and with T.  Appends the measured ratios to $TI_FF_FORCES_PARITY_OUT."""
    import torch
    worst_f = worst_e = 0.0
    full = {}
    n_full = max(batches)
    for n in batches:
        for temps, ref in ((None, ref0), (T, ref1)):
            tn = None if temps is None else temps[:n]
            F, S, E, Sb = (a[:n] for a in ref)
            f, e = eng.ff_forces(x[:n], to_nm, tn, energy=True)
            assert f.shape == (n, x.shape[1], 3) and f.dtype == np.float64 and np.isfinite(f).all() and np.isfinite(e).all()
            rf, re = float((np.abs(f - F) / S[..., None]).max()), float((np.abs(e - E) / Sb).max())
            worst_f, worst_e = max(worst_f, rf), max(worst_e, re)
            print(f"{name} B={n} T={'yes' if temps is not None else 'no'}: |dF| / S^F = {rf:.3e}, |dE| / S_b = {re:.3e}")
            assert (np.abs(f - F) <= TOL * S[..., None]).all(), (name, n, rf)
            assert (np.abs(e - E) <= TOL * Sb).all(), (name, n, re)
            # the exact force has no net force and no torque; every component of f is within TOL S^F of it (above), the restatement
            # within 1e-13 S^F: the sums are bounded by the sums of those bounds (2 TOL covers both)
            p = x[:n].astype(np.float64) * to_nm
            assert (np.abs(f.sum(axis=1)) <= 2 * TOL * S.sum(axis=1)[:, None]).all(), name
            lever = np.abs(p).max(axis=2)
            assert (np.abs(np.cross(p, f).sum(axis=1)) <= 4 * TOL * (lever * S).sum(axis=1)[:, None]).all(), name
            np.testing.assert_array_equal(bits(eng.ff_forces(x[:n], to_nm, tn)), bits(f))           # energy off: the same bits
            f2, e2 = eng.ff_forces(x[:n], to_nm, tn, energy=True)                                    # the same call twice
            np.testing.assert_array_equal(bits(f2), bits(f)); np.testing.assert_array_equal(bits(e2), bits(e))
            xd, td = torch.from_numpy(x[:n]).cuda(), (None if tn is None else torch.from_numpy(tn).cuda())
            fd, ed = eng.ff_forces(xd, to_nm, td, energy=True)                                       # device memory
            assert fd.is_cuda and fd.dtype == torch.float64 and tuple(fd.shape) == (n, x.shape[1], 3)
            np.testing.assert_array_equal(bits(fd.cpu().numpy()), bits(f)); np.testing.assert_array_equal(bits(ed.cpu().numpy()), bits(e))
            if n == n_full:
                full[temps is None] = (f, e)
    xf = x[:n_full]
    for temps in (None, T):
        tf = None if temps is None else temps[:n_full]
        f, e = full[temps is None]
        for b in alone:                                                                              # molecule b alone
            fb, eb = eng.ff_forces(xf[b:b + 1], to_nm, None if tf is None else tf[b:b + 1], energy=True)
            assert (bits(fb)[0] == bits(f)[b]).all() and bits(eb)[0] == bits(e)[b]
        fr, er = eng.ff_forces(np.ascontiguousarray(xf[::-1]), to_nm, None if tf is None else np.ascontiguousarray(tf[::-1]), energy=True)
        np.testing.assert_array_equal(bits(fr[::-1]), bits(f)); np.testing.assert_array_equal(bits(er[::-1]), bits(e))
        for n in [n for n in batches if n < n_full]:                                                 # the batch size does not enter
            np.testing.assert_array_equal(bits(eng.ff_forces(x[:n], to_nm, None if tf is None else tf[:n])), bits(f[:n]))
    out = os.environ.get("TI_FF_FORCES_PARITY_OUT")
    if out:
        with open(out, "a") as fh:
            fh.write(f"{name:4s} bonds {len(ff['bond_idx']):3d} angles {len(ff['angle_idx']):3d} torsions {len(ff['torsion_idx']):3d} "
                     f"pairs {x.shape[1] * (x.shape[1] - 1) // 2:3d}  largest |GPU - numpy| / S^F = {worst_f:.3e}, |dE| / S_b = {worst_e:.3e}\n")


@pytest.mark.parametrize("name", ["A2", "A4", "A9", "A25"])
def test_force_parity_and_bitwise_contract(name):
    pytest.importorskip("torch")
    eng, x, to_nm, T, ref0, ref1 = with_ff(name)
    check_forces(name, eng, cases()[name][0], x, to_nm, T, ref0, ref1)


def test_scalar_temperature_and_the_observables_entry():
    eng, x, to_nm, T, _, _ = with_ff("A9")
    np.testing.assert_array_equal(bits(eng.ff_forces(x[:5], to_nm, 300.0)), bits(eng.ff_forces(x[:5], to_nm, np.full(5, 300.0, np.float32))))
    f, e = pkg().observables.ff_forces(eng, x[:5], to_nm=to_nm, energy=True)
    assert f.dtype == np.float64 and f.shape == (5, 9, 3) and e.shape == (5,)
    # the reduced force is the force over R T
    fr = eng.ff_forces(x[:5], to_nm, T[:5])
    np.testing.assert_allclose(fr, f / (fn.R_GAS * T[:5].astype(np.float64))[:, None, None], rtol=4e-16, atol=0)


def test_nan_coordinate_and_coinciding_atoms_poison_their_molecule_only():
    eng, x, to_nm, T, _, _ = with_ff("A9")
    clean, clean_e = eng.ff_forces(x[:5], to_nm, T[:5], energy=True)
    bad = x[:5].copy()
    bad[3, 4, 1] = np.nan
    f, e = eng.ff_forces(bad, to_nm, T[:5], energy=True)
    assert np.isnan(f[3]).any() and np.isnan(e[3]) and np.isfinite(np.delete(f, 3, axis=0)).all()
    keep = [0, 1, 2, 4]
    np.testing.assert_array_equal(bits(f[keep]), bits(clean[keep])); np.testing.assert_array_equal(bits(e[keep]), bits(clean_e[keep]))
    ff = cases()["A9"][0]
    tab = fn.pair_table(ff, 9)
    i, j = next((i, j) for i in range(9) for j in range(i + 1, 9) if tab[fn.pair_row(i, j, 9), 2] > 0)
    hit = x[:2].copy()
    hit[1, j] = hit[1, i]
    f, e = eng.ff_forces(hit, to_nm, energy=True)
    assert not np.isfinite(f[1, i]).all() and not np.isfinite(f[1, j]).all() and e[1] == np.inf
    np.testing.assert_array_equal(bits(f[0]), bits(eng.ff_forces(x[:1], to_nm))[0])
    assert not np.isfinite(ffn.forces(hit, to_nm, ff)[0][1, i]).all()


def raw_forces(h, x, T=None, mem=0):
    """ti_obs_ff_forces on host memory with poisoned outputs; -> (return code, f, e)"""
    ti = pkg()
    B = x.shape[0]
    f, e = np.full(x.shape, -7.0), np.full(B, -7.0)
    rc = ti._lib.lib().ti_obs_ff_forces(h, C.c_void_p(x.ctypes.data), B, 0.125, None if T is None else C.c_void_p(T.ctypes.data),
                                        C.c_void_p(f.ctypes.data), C.c_void_p(e.ctypes.data), mem)
    return rc, f, e


def test_refusals_leave_the_outputs_untouched():
    ti = pkg()
    ARG, UNS = ti._lib.TI_E_ARG, ti._lib.TI_E_UNSUPPORTED
    eng, x, to_nm, T, _, _ = with_ff("A9")
    x5 = np.ascontiguousarray(x[:5])
    untouched = lambda f, e: (f == -7.0).all() and (e == -7.0).all()
    rc, f, e = raw_forces(eng.h, x5)
    assert rc == 0 and not untouched(f, e)
    for value in (0.0, -300.0, np.nan, np.inf):                                                     # found on the device
        Tb = np.full(5, 300.0, np.float32)
        Tb[2], Tb[4] = value, value
        rc, f, e = raw_forces(eng.h, x5, Tb)
        assert rc == ARG and "index 2" in ti._lib.last_error() and untouched(f, e), value
    rc, f, e = raw_forces(eng.h, x5, mem=7)
    assert rc == ARG and "mem" in ti._lib.last_error() and untouched(f, e)
    adw = ti.observables._service_engine(0)
    rc, f, e = raw_forces(adw.h, x5)
    assert rc == ARG and untouched(f, e)
    assert ti._lib.lib().ti_obs_ff_forces(None, None, 1, 1.0, None, None, None, 0) == ARG
    eng.set_molecules(np.full(5, 9, np.int32))
    try:
        rc, f, e = raw_forces(eng.h, x5)
        assert rc == UNS and untouched(f, e)
    finally:
        eng.set_molecules(None)
    eng.set_forcefield(None)
    rc, f, e = raw_forces(eng.h, x5)
    assert rc == ARG and "force field" in ti._lib.last_error() and untouched(f, e)
