"""ti_obs_ff_set / ti_obs_ff_energy / ti_obs_ti_logw on the GPU against the numpy restatement (tests/ff_numpy.py): parity of the total
and of every term column to 1e-11 S_b (S_b = sum over the evaluated terms of 1 + |term|; tests/test_forcefield.py holds the restatement
itself to 1e-13 S_b against 80-bit arithmetic on the same fixtures), the bitwise contract (repeat, alone, reversed, host against
device memory), the refusals with their outputs untouched, the log-weights bit for bit, and sample_ambient with the energy key.

Largest |GPU - numpy| / S_b per case, MI355X: profiles/ff_energy_parity.txt."""
import ctypes as C
import functools
import os
import types

import numpy as np
import pytest

from conftest import pkg
import ff_numpy as fn
from test_forcefield import gpu_fixtures

pytestmark = pytest.mark.gpu

TOL = 1e-11
B_FULL = 67
BATCHES = (1, 5, B_FULL)          # one molecule; fewer than a workgroup's four; not a multiple of four
RATIOS = {}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def engine(A):
    """A PaiNN handle for A atoms (the smallest model: the force field needs the handle's species size only)"""
    ti = pkg()
    syn, W = ti.synthetic, ti.weights
    src, dst, et = syn.fully_connected_template(A)
    flat = W.flatten_state_dict(syn.painn_state_dict(0, 32, 1, 25, seed=1), W.painn_param_spec(0, 32, 1, 25))
    return ti.engine.PainnEngine(0, 32, 1, A, src, dst, et, np.arange(A), flat, temp_length=100.0)


def trimmed(ff, n):
    out = dict(ff)
    out["torsion_idx"], out["torsion_par"] = ff["torsion_idx"][:n], ff["torsion_par"][:n]
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (force field dict, x [67, A, 3], to_nm, T [67], reference without T, reference with T); references computed once"""
    fx = {n: (ff, x, to_nm) for n, ff, x, to_nm in gpu_fixtures()}
    ff25, x25, nm25 = fx["A25"]
    fx["A25_t64"], fx["A25_t65"] = (trimmed(ff25, 64), x25, nm25), (trimmed(ff25, 65), x25, nm25)
    T = np.where(np.arange(B_FULL) % 2, 1000.0, 300.0).astype(np.float32)
    out = {}
    for name, (ff, x, to_nm) in fx.items():
        refs = []
        for temps in (None, T):
            E, sums, S, _ = fn.energies(x, to_nm, ff, T=temps)
            S = S if temps is None else S / (fn.R_GAS * temps.astype(np.float64))[:, None]
            refs.append((E, sums, S))
        out[name] = (ff, x, to_nm, T, refs[0], refs[1])
    return out


def with_ff(name):
    ti = pkg()
    ff, x, to_nm, T, r0, r1 = cases()[name]
    eng = engine(x.shape[1])
    eng.set_forcefield(ti.forcefield.ForceField(**ff))
    return eng, x, to_nm, T, r0, r1


def check(name, e, terms, ref, n):
    E, sums, S = (a[:n] for a in ref)
    assert np.isfinite(e).all()
    r = np.abs(e - E) / S.sum(axis=1)
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(r.max()))
    assert (np.abs(e - E) <= TOL * S.sum(axis=1)).all(), (name, r.max())
    if terms is not None:
        d = np.abs(terms - sums)
        RATIOS[name] = max(RATIOS[name], float((d / np.maximum(S, 1.0)).max()))
        assert (d <= TOL * S).all(), (name, (d / np.maximum(S, 1.0)).max(axis=0))
        np.testing.assert_array_equal(bits(e), bits(((terms[:, 0] + terms[:, 1]) + terms[:, 2]) + terms[:, 3]))


def check_energies(name, eng, x, to_nm, T, ref0, ref1, batches=BATCHES, alone=(0, 3, 4, 65, 66)):
    """The parity and the bitwise contract of ti_obs_ff_energy for one species: x [n, A, 3] with n = the largest of `batches`, the
    references (E, sums, S) without and with T"""
    import torch
    full = {}
    n_full = max(batches)
    for n in batches:
        for temps, ref in ((None, ref0), (T, ref1)):
            tn = None if temps is None else temps[:n]
            e, terms = eng.ff_energy(x[:n], to_nm, tn, terms=True)
            check(name, e, terms, ref, n)
            e_only = eng.ff_energy(x[:n], to_nm, tn)                                             # terms off: the same bits
            np.testing.assert_array_equal(bits(e_only), bits(e))
            e2, terms2 = eng.ff_energy(x[:n], to_nm, tn, terms=True)                              # the same call twice
            np.testing.assert_array_equal(bits(e2), bits(e)); np.testing.assert_array_equal(bits(terms2), bits(terms))
            xd, td = torch.from_numpy(x[:n]).cuda(), (None if tn is None else torch.from_numpy(tn).cuda())
            ed, termsd = eng.ff_energy(xd, to_nm, td, terms=True)                                  # device memory
            assert ed.is_cuda and ed.dtype == torch.float64 and tuple(termsd.shape) == (n, 4)
            np.testing.assert_array_equal(bits(ed.cpu().numpy()), bits(e)); np.testing.assert_array_equal(bits(termsd.cpu().numpy()), bits(terms))
            np.testing.assert_array_equal(bits(eng.ff_energy(xd, to_nm, td).cpu().numpy()), bits(e))
            if n == n_full:
                full[temps is None] = (e, terms)
    xf = x[:n_full]
    for temps in (None, T):
        tf = None if temps is None else temps[:n_full]
        e, terms = full[temps is None]
        for b in alone:                                                                            # molecule b alone
            eb, tb = eng.ff_energy(xf[b:b + 1], to_nm, None if tf is None else tf[b:b + 1], terms=True)
            assert bits(eb)[0] == bits(e)[b] and (bits(tb)[0] == bits(terms)[b]).all()
        er, tr = eng.ff_energy(np.ascontiguousarray(xf[::-1]), to_nm, None if tf is None else np.ascontiguousarray(tf[::-1]), terms=True)
        np.testing.assert_array_equal(bits(er[::-1]), bits(e)); np.testing.assert_array_equal(bits(tr[::-1]), bits(terms))
        for n in [n for n in batches if n < n_full]:                                               # the batch size does not enter
            np.testing.assert_array_equal(bits(eng.ff_energy(x[:n], to_nm, None if tf is None else tf[:n])), bits(e[:n]))
    print(f"{name}: largest |GPU - numpy| / S_b = {RATIOS[name]:.3e} (bound {TOL:.0e})")


@pytest.mark.parametrize("name", ["A2", "A4", "A9", "A25", "A25_t64", "A25_t65"])
def test_energy_parity_and_bitwise_contract(name):
    pytest.importorskip("torch")
    eng, x, to_nm, T, ref0, ref1 = with_ff(name)
    check_energies(name, eng, x, to_nm, T, ref0, ref1)
    out = os.environ.get("TI_FF_PARITY_OUT")
    if out:
        with open(out, "a") as f:
            ff = cases()[name][0]
            f.write(f"{name:8s} bonds {len(ff['bond_idx']):3d} angles {len(ff['angle_idx']):3d} torsions {len(ff['torsion_idx']):3d} "
                    f"pairs {x.shape[1] * (x.shape[1] - 1) // 2:3d}  largest |GPU - numpy| / S_b = {RATIOS[name]:.3e}\n")


def test_a_scalar_temperature_is_every_molecules():
    eng, x, to_nm, T, _, _ = with_ff("A9")
    np.testing.assert_array_equal(bits(eng.ff_energy(x[:5], to_nm, 300.0)), bits(eng.ff_energy(x[:5], to_nm, np.full(5, 300.0, np.float32))))
    assert pkg().observables.ff_energy(eng, x[:5], to_nm=to_nm).dtype == np.float64


def test_nan_coordinate_and_coinciding_atoms():
    eng, x, to_nm, T, _, _ = with_ff("A9")
    clean, clean_t = eng.ff_energy(x[:5], to_nm, T[:5], terms=True)
    bad = x[:5].copy()
    bad[3, 4, 1] = np.nan
    e, terms = eng.ff_energy(bad, to_nm, T[:5], terms=True)
    assert np.isnan(e[3]) and np.isfinite(np.delete(e, 3)).all()
    keep = [0, 1, 2, 4]
    np.testing.assert_array_equal(bits(e[keep]), bits(clean[keep])); np.testing.assert_array_equal(bits(terms[keep]), bits(clean_t[keep]))
    # two atoms of an evaluated pair on one point: +inf, not an error (the wall wins whatever the charges are)
    ff = cases()["A9"][0]
    tab = fn.pair_table(ff, 9)
    i, j = next((i, j) for i in range(9) for j in range(i + 1, 9) if tab[fn.pair_row(i, j, 9), 2] > 0)
    hit = x[:2].copy()
    hit[1, j] = hit[1, i]
    e = eng.ff_energy(hit, to_nm)
    assert e[1] == np.inf and bits(e)[0] == bits(eng.ff_energy(x[:1], to_nm))[0]
    assert fn.energies(hit, to_nm, ff)[0][1] == np.inf


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def raw_set(eng, ff, A, **over):
    """ti_obs_ff_set through ctypes with single entries overridden; -> return code"""
    ti = pkg()
    t = {k: np.array(v, copy=True) for k, v in ff.items() if k != "coulomb"}
    t["pairs"] = fn.pair_table(ff, A)
    for k, fnc in over.items():
        t[k] = fnc(t[k])
    t = {k: np.ascontiguousarray(v, np.int32 if k.endswith("idx") else np.float64) for k, v in t.items()}
    desc = ti._lib.FfDesc(len(t["bond_idx"]), len(t["angle_idx"]), len(t["torsion_idx"]), len(t["pairs"]), fn.COULOMB)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    return ti._lib.lib().ti_obs_ff_set(eng.h, C.byref(desc), ip(t["bond_idx"]), dp(t["bond_par"]), ip(t["angle_idx"]), dp(t["angle_par"]),
                                       ip(t["torsion_idx"]), dp(t["torsion_par"]), dp(t["pairs"]))


def raw_energy(h, x, T=None):
    """ti_obs_ff_energy on host memory with poisoned outputs; -> (return code, e, terms)"""
    ti = pkg()
    B = x.shape[0]
    e, terms = np.full(B, -7.0), np.full((B, 4), -7.0)
    rc = ti._lib.lib().ti_obs_ff_energy(h, C.c_void_p(x.ctypes.data), B, 0.125, None if T is None else C.c_void_p(T.ctypes.data),
                                        C.c_void_p(e.ctypes.data), C.c_void_p(terms.ctypes.data), 0)
    return rc, e, terms


def setter(row, col, value):
    def f(a):
        a[row, col] = value
        return a
    return f


def test_refusals_leave_the_outputs_and_the_force_field_untouched():
    ti = pkg()
    L, ARG, UNS = ti._lib.lib(), ti._lib.TI_E_ARG, ti._lib.TI_E_UNSUPPORTED
    eng, x, to_nm, T, _, _ = with_ff("A9")
    ff = cases()["A9"][0]
    x5 = np.ascontiguousarray(x[:5])
    before = eng.ff_energy(x5, 0.125)
    untouched = lambda e, terms: (e == -7.0).all() and (terms == -7.0).all()
    assert raw_set(eng, ff, 9) == 0
    grow = lambda a: np.concatenate([a] * (513 // len(a) + 1))[:513]
    bad_sets = {"an index equal to A": dict(angle_idx=setter(1, 2, 9)), "a negative index": dict(bond_idx=setter(0, 0, -1)),
                "a repeated atom": dict(torsion_idx=lambda a: setter(2, 3, a[2, 0])(a)), "n = 7": dict(torsion_par=setter(0, 0, 7.0)),
                "n = 0": dict(torsion_par=setter(0, 0, 0.0)), "n = 2.5": dict(torsion_par=setter(0, 0, 2.5)),
                "a NaN parameter": dict(bond_par=setter(3, 1, np.nan)), "an infinite phase": dict(torsion_par=setter(1, 1, np.inf)),
                "sigma < 0": dict(pairs=setter(4, 1, -0.1)), "eps < 0": dict(pairs=setter(4, 2, -0.1)), "a NaN charge product": dict(pairs=setter(0, 0, np.nan)),
                "513 torsions": dict(torsion_idx=grow, torsion_par=grow), "65 bonds": dict(bond_idx=lambda a: np.concatenate([a] * 9)[:65], bond_par=lambda a: np.concatenate([a] * 9)[:65]),
                "a short pair table": dict(pairs=lambda a: a[:-1])}
    for what, over in bad_sets.items():
        assert raw_set(eng, ff, 9, **over) == ARG, what
        assert ti._lib.last_error(), what
        np.testing.assert_array_equal(bits(eng.ff_energy(x5, 0.125)), bits(before), err_msg=what)      # the force field in force stays
    # temperatures: found on the device, the message names the first bad index
    for value in (0.0, -300.0, np.nan, np.inf):
        Tb = np.full(5, 300.0, np.float32)
        Tb[2], Tb[4] = value, value
        rc, e, terms = raw_energy(eng.h, x5, Tb)
        assert rc == ARG and "index 2" in ti._lib.last_error() and untouched(e, terms), value
    # an adw handle
    adw = ti.observables._service_engine(0)
    assert raw_set(adw, ff, 9) == ARG
    rc, e, terms = raw_energy(adw.h, x5)
    assert rc == ARG and untouched(e, terms)
    assert L.ti_obs_ff_set(None, None, None, None, None, None, None, None, None) == ARG
    # ti_painn_set_molecules in force: one force field is one species
    eng.set_molecules(np.full(5, 9, np.int32))
    try:
        assert raw_set(eng, ff, 9) == UNS
        rc, e, terms = raw_energy(eng.h, x5)
        assert rc == UNS and untouched(e, terms)
    finally:
        eng.set_molecules(None)
    np.testing.assert_array_equal(bits(eng.ff_energy(x5, 0.125)), bits(before))
    # cleared with desc == NULL, and a handle that never had one
    eng.set_forcefield(None)
    rc, e, terms = raw_energy(eng.h, x5)
    assert rc == ARG and "force field" in ti._lib.last_error() and untouched(e, terms)
    fresh = engine(3)                                                                               # no ti_obs_ff_set yet on this handle
    rc, e, terms = raw_energy(fresh.h, np.zeros((2, 3, 3), np.float32))
    assert rc == ARG and untouched(e, terms)


# ---- log-weights ---------------------------------------------------------------------------------------------------------------
def test_ti_logw_bit_for_bit_and_into_the_weights():
    torch = pytest.importorskip("torch")
    ti = pkg()
    rs = np.random.RandomState(5)
    B = B_FULL
    u0, u1, nd = rs.standard_normal(B) * 40.0 + 900.0, rs.standard_normal(B) * 40.0 + 900.0, (rs.standard_normal(B) * 3.0).astype(np.float32)
    eng = ti.observables._service_engine(0)
    zero = np.zeros(B)
    for a, n in ((u0, nd), (None, nd), (u0, None), (None, None)):
        want = np.float32(-(u1 - (zero if a is None else a) + np.float64(zero if n is None else n)))
        got = ti.observables.ti_logw(a, u1, n)
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
        dev = lambda v: None if v is None else torch.from_numpy(v).cuda()
        got_d = eng.ti_logw(dev(a), dev(u1), dev(n))
        assert got_d.is_cuda and got_d.dtype == torch.float32
        np.testing.assert_array_equal(got_d.cpu().numpy().view(np.uint32), want.view(np.uint32))
    want = np.float32(-(u1 - u0 + np.float64(nd)))
    w_d, ess_d = eng.importance_weights(eng.ti_logw(*(torch.from_numpy(v).cuda() for v in (u0, u1, nd))))
    w, ess = ti.observables.importance_weights(want)
    assert ess_d == ess and np.array_equal(w_d.cpu().numpy().view(np.uint32), w.view(np.uint32))
    # non-finite inputs pass through; the consumer refuses them by index
    u1n = u1.copy()
    u1n[7] = np.nan
    lw = ti.observables.ti_logw(u0, u1n, nd)
    assert np.isnan(lw[7]) and np.isfinite(np.delete(lw, 7)).all()
    with pytest.raises(ti._lib.TiError, match="index 7"):
        ti.observables.importance_weights(lw)
    assert ti._lib.lib().ti_obs_ti_logw(eng.h, None, None, None, B, None, 0) == ti._lib.TI_E_ARG


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def write_xml(ff, path):
    """the synthetic species as the XML OpenMM's serializer writes (the attributes the reader takes)"""
    rows = lambda tag, items: "".join(f"<{tag} " + " ".join(f'{k}="{v!r}"' for k, v in it.items()) + "/>" for it in items)
    f = lambda v: float(v)
    bonds = [dict(p1=int(i), p2=int(j), d=f(d), k=f(k)) for (i, j), (d, k) in zip(ff["bond_idx"], ff["bond_par"])]
    angles = [dict(p1=int(i), p2=int(j), p3=int(k), a=f(a), k=f(kk)) for (i, j, k), (a, kk) in zip(ff["angle_idx"], ff["angle_par"])]
    tors = [dict(p1=int(i), p2=int(j), p3=int(k), p4=int(l), periodicity=int(n), phase=f(ph), k=f(kk))
            for (i, j, k, l), (n, ph, kk) in zip(ff["torsion_idx"], ff["torsion_par"])]
    parts = [dict(q=f(q), sig=f(s), eps=f(e)) for q, s, e in ff["particles"]]
    excs = [dict(p1=int(i), p2=int(j), q=f(q), sig=f(s), eps=f(e)) for i, j, q, s, e in ff["exceptions"]]
    text = ("<System><Particles>" + '<Particle mass="1"/>' * len(parts) + "</Particles><Forces>"
            f'<Force type="HarmonicBondForce"><Bonds>{rows("Bond", bonds)}</Bonds></Force>'
            f'<Force type="HarmonicAngleForce"><Angles>{rows("Angle", angles)}</Angles></Force>'
            f'<Force type="PeriodicTorsionForce"><Torsions>{rows("Torsion", tors)}</Torsions></Force>'
            f'<Force type="NonbondedForce" method="0"><GlobalParameters/><ParticleOffsets/><ExceptionOffsets/>'
            f'<Particles>{rows("Particle", parts)}</Particles><Exceptions>{rows("Exception", excs)}</Exceptions></Force>'
            '<Force type="CMMotionRemover"/></Forces></System>')
    with open(path, "w") as fh:
        fh.write(text)


def test_sample_ambient_with_the_energy_key(tmp_path):
    ti = pkg()
    ff, x, to_nm, _, _, _ = cases()["A9"]
    A, n, scale = 9, 12, 1.0 / to_nm
    write_xml(ff, tmp_path / "ff.xml")
    parsed = ti.forcefield.ForceField.from_openmm_xml(str(tmp_path / "ff.xml"))
    np.testing.assert_array_equal(parsed.pair_table(), fn.pair_table(ff, A))
    traj = np.zeros((8, n, A, 3))
    # the T0 = 1000 K slot: one geometry with 3e-5 nm of noise, which spreads phi by about 1 (the bonds are stiff): the ESS of the
    # 12 samples is then neither 1 nor 12
    traj[7] = x[0].astype(np.float64) + np.random.RandomState(8).standard_normal((n, A, 3)) * 3e-5 * scale
    os.makedirs(tmp_path / "test")
    np.save(tmp_path / "test" / "00031.npy", traj)
    ds = ti.data.MDQM9SamplerDataset("00031.npy", str(tmp_path), "test", T0=1000, T1=300, scale=False, cutoff=1000)
    b = ti.thermo.ambient.cPaiNN(n_features=32, score_layers=1, temp_length=100)
    b.load_state_dict(ti.synthetic.painn_state_dict(0, 32, 1, 25, 4))
    obs = {"descriptors": [["dist", 0, 1], ["torsion", 0, 1, 2, 3]], "bins": 4, "bootstrap": 16}
    common = dict(seed=0, batch_size=6, n_steps=3, atol=1e-5, rtol=1e-5, return_dlogp=1, method="euler")
    plain = types.SimpleNamespace(**common, data_save_path=str(tmp_path / "plain"), data_save_name="p", observables=obs)
    ti.drivers.sample_ambient(plain, b, ds)
    assert sorted(os.listdir(tmp_path / "plain")) == ["dlogps_p.npy", "latent_dlogps_p.npy", "latent_noises_p.npy", "observables_p.npz", "samples_p.npy"]
    with np.load(tmp_path / "plain" / "observables_p.npz") as z:
        assert sorted(z.files) == ["cv", "edges", "ess", "ess_boot", "ess_ci", "hist"]
        ess_plain = float(z["ess"])
    cfg = types.SimpleNamespace(**common, data_save_path=str(tmp_path / "out"), data_save_name="e",
                                observables={**obs, "energy": {"forcefield": str(tmp_path / "ff.xml"), "scale": scale}})
    samples, _ = ti.drivers.sample_ambient(cfg, b, ds)
    out = tmp_path / "out"
    E0, E1, dl = np.load(out / "E0s_samples_e.npy"), np.load(out / "E1s_samples_e.npy"), np.load(out / "dlogps_e.npy")
    assert E0.shape == E1.shape == (n,) and E0.dtype == np.float64 and np.isfinite(E0).all() and np.isfinite(E1).all()
    np.testing.assert_array_equal(samples.view(np.uint32), np.load(tmp_path / "plain" / "samples_p.npy").view(np.uint32))
    # the written energies are those of the written samples: x0 at T0 = 1000 K, the end state at T1 = 300 K
    for E, frame, temp in ((E0, 0, 1000.0), (E1, -1, 300.0)):
        ref, _, S, _ = fn.energies(samples[:, frame], to_nm, ff, T=np.full(n, temp, np.float32))
        assert (np.abs(E - ref) <= TOL * S.sum(axis=1) / (fn.R_GAS * temp)).all()
    with np.load(out / "observables_e.npz") as z:
        assert sorted(z.files) == sorted(["cv", "edges", "ess", "ess_boot", "ess_ci", "hist", "E0", "E1", "logw", "ess_ti", "ess_ti_ci"])
        assert float(z["ess"]) == ess_plain                      # keeps its meaning and its value
        np.testing.assert_array_equal(z["E0"], E0); np.testing.assert_array_equal(z["E1"], E1)
        phi = E1 - E0 + dl.astype(np.float64)                    # the reference's weights exp(-(E1 - E0 + neg_dlogp)), calc_ESS with a shift
        np.testing.assert_array_equal(z["logw"].view(np.uint32), np.float32(-phi).view(np.uint32))
        lw = np.float32(-phi).astype(np.float64)                 # the weights are taken from the fp32 logw
        w = np.exp(lw - lw.max())
        want = np.square(w.sum()) / np.square(w).sum()
        assert abs(float(z["ess_ti"]) - want) <= 1e-6 * want
        lo, hi = z["ess_ti_ci"]
        assert 1.0 <= lo <= hi <= n
        print(f"ess (dlogp only) {ess_plain:.3f}, ess_ti {float(z['ess_ti']):.3f} (reference formula {want:.3f}), ci [{lo:.3f}, {hi:.3f}]")
