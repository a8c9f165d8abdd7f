"""Force fields on the host: known answers of the numpy restatement (tests/ff_numpy.py), the dense pair table, the OpenMM XML reader
with its refusals, and the conditioning of the fixtures the GPU tests compare on (fp64 against np.longdouble).  No GPU."""
import os
import types

import numpy as np
import pytest

from conftest import GOLDEN, pkg
import ff_numpy as fn

XML = os.path.join(GOLDEN, "ff_small.xml")


def empty_ff(A, **kw):
    ff = dict(bond_idx=np.zeros((0, 2), np.int32), bond_par=np.zeros((0, 2)), angle_idx=np.zeros((0, 3), np.int32), angle_par=np.zeros((0, 2)),
              torsion_idx=np.zeros((0, 4), np.int32), torsion_par=np.zeros((0, 3)), particles=np.zeros((A, 3)), exceptions=np.zeros((0, 5)),
              coulomb=fn.COULOMB)
    ff.update(kw)
    return ff


def single(x, ff, column):
    E, sums, _, _ = fn.energies(np.asarray(x, np.float32)[None], 1.0, ff)
    assert E[0] == sums[0, column] and (np.delete(sums[0], column) == 0).all()
    return E[0]


def close(a, b):
    return abs(a - b) <= 1e-15 * abs(b)


# ---- 1. known answers ----------------------------------------------------------------------------------------------------------
def test_known_answers():
    r, r0, k = 0.25, 0.125, 1000.0                            # exact in fp32 and fp64
    assert close(single([[0, 0, 0], [r, 0, 0]], empty_ff(2, bond_idx=[[0, 1]], bond_par=[[r0, k]]), 0), k * (r - r0) ** 2 / 2)
    right = [[1, 0, 0], [0, 0, 0], [0, 2, 0]]
    assert close(single(right, empty_ff(3, angle_idx=[[0, 1, 2]], angle_par=[[1.9, k]]), 1), k * (np.pi / 2 - 1.9) ** 2 / 2)
    # the torsion formula at phi = pi / 3 as fp64 holds it: n = 3, phase 0 gives 0; n = 1, phase pi gives k / 2
    phi = np.pi / 3
    assert fn.torsion_energy(phi, 3.0, 0.0, k) == 0.0
    assert close(fn.torsion_energy(phi, 1.0, np.pi, k), k / 2)
    # and through a geometry whose torsion is pi / 3 to the fp32 coordinates: b1 = -x, b2 = z, b3 at 60 degrees in the xy plane
    tors = np.array([[1, 0, 0], [0, 0, 0], [0, 0, 1], [0.5, np.sqrt(3) / 2, 1]], np.float32)
    assert abs(single(tors, empty_ff(4, torsion_idx=[[0, 1, 2, 3]], torsion_par=[[3, 0.0, k]]), 2)) < 1e-10 * k          # 1 + cos(pi + 1e-7)
    assert abs(single(tors, empty_ff(4, torsion_idx=[[0, 1, 2, 3]], torsion_par=[[1, np.pi, k]]), 2) - k / 2) < 1e-6 * k
    unit = empty_ff(2, particles=[[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    assert close(single([[0, 0, 0], [1, 0, 0]], unit, 3), 138.935456)
    sigma, eps = 0.25, 0.75
    lj = empty_ff(2, particles=[[0.0, sigma, eps], [0.0, sigma, eps]])
    r = 2.0 ** (1.0 / 6.0) * sigma
    x = np.zeros((1, 2, 3), np.float32)
    x[0, 1, 0] = 1.0
    E, _, _, _ = fn.energies(x, r, lj)                        # the distance through to_nm: exact in fp64, not rounded to fp32
    assert abs(E[0] + eps) <= 4e-15 * eps                     # (sigma / r)^6 = 1 / 2 to 3 ulp: 6 roundings of the sixth power


def test_degenerate_geometry_in_the_restatement():
    ff = empty_ff(2, particles=[[1.0, 0.25, 0.5], [-1.0, 0.25, 0.5]])
    assert fn.energies(np.zeros((1, 2, 3), np.float32), 1.0, ff)[0][0] == np.inf               # the wall wins over the attraction
    x = np.zeros((2, 2, 3), np.float32)
    x[:, 1, 0] = 1.0
    x[1, 0, 2] = np.nan
    E = fn.energies(x, 1.0, ff)[0]
    assert np.isfinite(E[0]) and np.isnan(E[1])


# ---- 2. pair table -------------------------------------------------------------------------------------------------------------
def test_pair_table():
    ti = pkg()
    A = 7
    ffd = fn.chain_forcefield(A, 3)
    ff = ti.forcefield.ForceField(**ffd)
    tab = ff.pair_table(A)
    assert tab.shape == (21, 3) and tab.dtype == np.float64
    np.testing.assert_array_equal(tab, fn.pair_table(ffd, A))
    rows = [(i, j) for i in range(A) for j in range(i + 1, A)]                  # row order
    assert [ti.forcefield.pair_row(i, j, A) for i, j in rows] == list(range(21))
    exc = {(int(e[0]), int(e[1])): e[2:] for e in ffd["exceptions"]}
    q, sig, eps = ffd["particles"].T
    zeroed = 0
    for k, (i, j) in enumerate(rows):
        if (i, j) in exc:
            np.testing.assert_array_equal(tab[k], exc[(i, j)])                 # the override
            zeroed += tab[k, 0] == 0 and tab[k, 2] == 0
        else:
            np.testing.assert_array_equal(tab[k], [q[i] * q[j], (sig[i] + sig[j]) / 2, np.sqrt(eps[i] * eps[j])])
    assert zeroed == sum(1 for e in exc.values() if e[0] == 0 and e[2] == 0) >= A - 1         # every bond at least
    assert len(exc) == 6 + 5 + 4                                                # 1-2, 1-3, 1-4 of a chain; the other 6 pairs keep the combination rule
    # an exception listed as (j, i) lands in the row of (i, j)
    ff2 = ti.forcefield.ForceField(particles=ffd["particles"], exceptions=[[3, 1, 0.5, 0.2, 0.1]])
    assert ff2.pair_table(A)[ti.forcefield.pair_row(1, 3, A)].tolist() == [0.5, 0.2, 0.1]
    with pytest.raises(ValueError):
        ff.pair_table(A + 1)


# ---- 3. the OpenMM XML reader --------------------------------------------------------------------------------------------------
def test_from_openmm_xml_reads_every_table():
    ti = pkg()
    ff = ti.forcefield.ForceField.from_openmm_xml(XML)
    assert ff.n_atoms == 5 and ff.coulomb == 138.935456
    assert ff.bond_idx.tolist() == [[0, 1], [1, 2], [2, 3], [2, 4]]
    np.testing.assert_array_equal(ff.bond_par, [[0.1526, 259408.0], [0.1449, 282001.6], [0.1229, 476976.0], [0.101, 363171.2]])
    assert ff.angle_idx.tolist() == [[0, 1, 2], [1, 2, 3], [1, 2, 4], [3, 2, 4]]
    np.testing.assert_array_equal(ff.angle_par[:, 1], [527.184, 669.44, 418.4, 292.88])
    assert ff.angle_par[3, 0] == 2.0943951023931953
    assert ff.torsion_idx.tolist() == [[0, 1, 2, 3], [0, 1, 2, 3], [0, 1, 2, 4]]                # two terms on one quadruple
    np.testing.assert_array_equal(ff.torsion_par, [[2, np.pi, 10.46], [1, 0.0, 8.368], [3, 0.0, 0.6508444444444444]])
    np.testing.assert_array_equal(ff.particles[:, 0], [-0.1825, 0.0337, -0.4157, -0.5679, 0.2719])
    assert ff.particles[4].tolist() == [0.2719, 0.1069078422195985, 0.0656888]
    assert ff.exceptions.shape == (10, 5) and ff.exceptions[8].tolist() == [4, 0, -0.041351458333333334, 0.223437396530976, 0.08670020699999999]
    tab = ff.pair_table()
    live = [(i, j) for i in range(5) for j in range(i + 1, 5) if tab[ti.forcefield.pair_row(i, j, 5)][[0, 2]].any()]
    assert live == [(0, 3), (0, 4)]                           # the 1-4 pairs; (3, 4) is a 1-3 pair
    text = open(XML).read()
    ff_t = ti.forcefield.ForceField.from_openmm_xml(text)     # the text itself
    np.testing.assert_array_equal(ff_t.pair_table(), tab)
    # the energy of the parsed force field is a number the restatement can form
    x = np.array([[[0, 0, 0], [0.15, 0, 0], [0.2, 0.13, 0], [0.32, 0.15, 0.02], [0.13, 0.21, -0.03]]], np.float32)
    E, sums, _, _ = fn.energies(x, 1.0, vars(ff))
    assert np.isfinite(E).all() and (sums[0, :3] > 0).all()


REFUSALS = [
    ("cutoff method", 'method="0" name="NonbondedForce"', 'method="1" name="NonbondedForce"', "NoCutoff"),
    ("PME method", 'method="0" name="NonbondedForce"', 'method="4" name="NonbondedForce"', "NoCutoff"),
    ("global parameter", "<GlobalParameters/>", '<GlobalParameters><Parameter default="1" name="lambda"/></GlobalParameters>', "GlobalParameters"),
    ("particle offset", "<ParticleOffsets/>", '<ParticleOffsets><Offset eps="0" parameter="lambda" particle="0" q="1" sig="0"/></ParticleOffsets>',
     "ParticleOffsets"),
    ("exception offset", "<ExceptionOffsets/>", '<ExceptionOffsets><Offset eps="0" exception="0" parameter="lambda" q="1" sig="0"/></ExceptionOffsets>',
     "ExceptionOffsets"),
    ("another force", 'name="CMMotionRemover" type="CMMotionRemover"', 'name="CustomBondForce" type="CustomBondForce"', "CustomBondForce"),
    ("a barostat", 'name="CMMotionRemover" type="CMMotionRemover"', 'name="MonteCarloBarostat" type="MonteCarloBarostat"', "MonteCarloBarostat"),
]


@pytest.mark.parametrize("what,old,new,named", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_from_openmm_xml_refusals(what, old, new, named):
    ti = pkg()
    text = open(XML).read()
    assert text.count(old) == 1
    with pytest.raises(ValueError, match=named):
        ti.forcefield.ForceField.from_openmm_xml(text.replace(old, new))


def test_from_openmm_xml_needs_a_system():
    ti = pkg()
    with pytest.raises(ValueError):
        ti.forcefield.ForceField.from_openmm_xml("<Nothing><Forces/></Nothing>")


# ---- 4. conditioning of the GPU fixtures ---------------------------------------------------------------------------------------
def gpu_fixtures():
    """(name, force field dict, x [67, A, 3] fp32, to_nm): the species the GPU parity tests use, generated once"""
    out = []
    for name, ff in (("A2", fn.chain_forcefield(2)), ("A4", fn.chain_forcefield(4)), ("A9", fn.synthetic_forcefield(9)),
                     ("A25", fn.synthetic_forcefield(25))):
        x, to_nm = fn.synthetic_geometry(ff, 67, seed=len(out) + 1)
        out.append((name, ff, x, to_nm))
    return out


def test_the_gpu_fixtures_have_the_shapes_their_cases_need():
    fx = {n: ff for n, ff, _, _ in gpu_fixtures()}
    assert [len(fx["A2"][k]) for k in ("bond_idx", "angle_idx", "torsion_idx")] == [1, 0, 0] and not fn.pair_table(fx["A2"], 2)[:, [0, 2]].any()
    assert [len(fx["A4"][k]) for k in ("bond_idx", "angle_idx", "torsion_idx")] == [3, 2, 1]
    t4 = fn.pair_table(fx["A4"], 4)
    assert [(r[0] != 0) or (r[2] != 0) for r in t4] == [False, False, True, False, False, False]         # one live 1-4 pair
    nt = len(fx["A25"]["torsion_idx"])
    assert 128 < nt <= 512 and nt % 64 and len(fx["A25"]["angle_idx"]) <= 128 and fn.pair_table(fx["A25"], 25).shape[0] == 300


def test_the_gpu_fixtures_are_well_conditioned():
    """|E64 - E80| <= 1e-13 S_b for the total and for every column: the restatement in fp64 against the same code in np.longdouble"""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than float64 here")
    T = np.where(np.arange(67) % 2, 1000.0, 300.0).astype(np.float32)
    worst = 0.0
    for name, ff, x, to_nm in gpu_fixtures():
        for temps in (None, T):
            E64, s64, S, _ = fn.energies(x, to_nm, ff, T=temps)
            E80, s80, _, _ = fn.energies(x, to_nm, ff, T=temps, ft=np.longdouble)
            S = S if temps is None else S / (fn.R_GAS * temps.astype(np.float64))[:, None]
            assert np.isfinite(E64).all()
            r_tot = np.abs((E64 - E80).astype(np.float64)) / S.sum(axis=1)
            r_col = np.abs((s64 - s80).astype(np.float64)) / np.maximum(S, 1.0)          # an empty table: S = 0 and the sums are exactly 0
            worst = max(worst, r_tot.max(), r_col.max())
            assert r_tot.max() <= 1e-13 and r_col.max() <= 1e-13, (name, r_tot.max(), r_col.max())
    print(f"fp64 against 80-bit: worst |dE| / S = {worst:.2e}")


# ---- the driver key, as far as it goes without a device ------------------------------------------------------------------------
def test_the_energy_key_is_checked_before_any_rollout(tmp_path):
    dr = pkg().drivers
    obs = {"descriptors": [["dist", 0, 1]], "energy": {"forcefield": XML, "scale": 10.0}}
    ff, to_nm = dr._check_energy(types.SimpleNamespace(observables=obs, return_dlogp=1))
    assert ff.n_atoms == 5 and to_nm == 0.1
    assert dr._check_energy(types.SimpleNamespace()) is None
    assert dr._check_energy(types.SimpleNamespace(observables={"descriptors": [["dist", 0, 1]]})) is None
    with pytest.raises(ValueError, match="return_dlogp"):
        dr._check_energy(types.SimpleNamespace(observables=obs, return_dlogp=0))
    for bad in ({"forcefield": XML}, {"forcefield": XML, "scale": 0.0}, {"forcefield": XML, "scale": 1.0, "extra": 1}, "x"):
        with pytest.raises(ValueError, match="energy"):
            dr._check_energy(types.SimpleNamespace(observables={**obs, "energy": bad}, return_dlogp=1))
    none = str(tmp_path / "none")
    with pytest.raises(ValueError, match="log p"):
        dr.sample_latent(types.SimpleNamespace(observables=obs, return_dlogp=1, data_save_path=none), None, None)
    with pytest.raises(ValueError, match="force field"):
        dr.sample_adw(types.SimpleNamespace(observables=obs, return_dlogp=1, beta0s=[1.0], beta1s=[1.25]), types.SimpleNamespace(dim=1), [])
    with pytest.raises(ValueError, match="return_dlogp"):
        dr.sample_ambient(types.SimpleNamespace(observables=obs, return_dlogp=0, data_save_path=none), None, None)
    assert not os.path.exists(none)
    assert "energy" not in dr._observe_kw(types.SimpleNamespace(observables=obs))["observe"]
