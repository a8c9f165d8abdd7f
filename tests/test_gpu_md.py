"""ti_obs_ff_langevin on the GPU against the numpy restatement (tests/ff_forces_numpy.py) and against physics: a 16-step Langevin
trajectory within 100 d64 of the restatement (d64: the restatement's own fp64 error against np.longdouble on the same run; the ratio
between the energy tests' GPU and restatement bars), the drawn velocities exactly, the bitwise contract (repeat, host against device
memory, alone, reversed, chained, launch cut, strides), energy conservation without a thermostat against the restatement's own
fluctuation, the bond-length distribution of a diatomic against quadrature, the failure path, the refusals, and drivers.generate_md
end to end.

Measured ratios, MI355X: profiles/md_parity.txt."""
import ctypes as C
import functools
import os
import types

import numpy as np
import pytest

from conftest import pkg
import ff_numpy as fn
import ff_forces_numpy as ffn
from test_forcefield import gpu_fixtures
from test_gpu_forcefield import engine, write_xml

pytestmark = pytest.mark.gpu

LD = np.longdouble


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


@functools.lru_cache(maxsize=None)
def species(name):
    ff, x, to_nm = next((ff, x, to_nm) for n, ff, x, to_nm in gpu_fixtures() if n == name)
    return ff, ffn.masses_for(ff), x, to_nm


def with_md(name, masses=None):
    ti = pkg()
    ff, m, x, to_nm = species(name)
    eng = engine(x.shape[1])
    eng.set_forcefield(ti.forcefield.ForceField(**ff, masses=m if masses is None else masses))
    return eng, ff, (m if masses is None else masses), x, to_nm


def case(name, B=5):
    eng, ff, m, x, to_nm = with_md(name)
    pos = x[:B].astype(np.float64) * to_nm
    T = np.where(np.arange(B) % 2, 1000.0, 300.0).astype(np.float32)
    ids = np.arange(B, dtype=np.int64) * 3 + 7
    return eng, ff, m, pos, T, ids, to_nm


RUN = dict(dt=5e-4, friction=1.0, n_steps=16, stride=4, seed=11)


# ---- the trajectory against the restatement ----------------------------------------------------------------------------------------
def check_trajectory(name, eng, ff, m, pos, T, ids, to_nm, run=RUN):
    """One run with drawn velocities against the restatement: the drawn velocities exactly, the state within 100 d64, the frames and
    their energies within the bounds derived below.  Appends the measured ratio to $TI_MD_PARITY_OUT; returns it."""
    B, n_frames = len(pos), run["n_steps"] // run["stride"]
    kw = dict(ff=ff, masses=m, to_nm=to_nm, draw=True, **run)
    p64, v64, f64, e64, k64 = ffn.langevin(pos, None, T, ids, **kw)
    p80, v80, _, _, _ = ffn.langevin(pos, None, T, ids, ft=LD, **kw)
    d64 = float(max(np.abs(p64 - p80).max(), np.abs(v64 - v80).max()))
    # the drawn velocities: sqrt(R T / m) times the Philox normal, correctly rounded operations only -- exactly the restatement's
    _, v0, _, _, _ = eng.langevin(pos, None, T, run["dt"], run["friction"], 0, seed=run["seed"], ids=ids, to_nm=to_nm, draw_velocities=True)
    np.testing.assert_array_equal(bits(v0), bits(ffn.draw_velocities(T, ids, m, run["seed"], 0)))
    p, v, fr, ep, ek = eng.langevin(pos, None, T, run["dt"], run["friction"], run["n_steps"], stride=run["stride"], seed=run["seed"], ids=ids,
                                    to_nm=to_nm, draw_velocities=True)
    assert fr.shape == (B, n_frames, pos.shape[1], 3) and fr.dtype == np.float32 and ep.shape == ek.shape == (B, n_frames)
    assert np.isfinite(p).all() and np.isfinite(v).all()
    dp, dv = float(np.abs(p - p64).max()), float(np.abs(v - v64).max())
    # a frame is the fp64 value rounded once to fp32: within the state's bar in model units, plus one fp32 rounding step of the value
    tol_f = 100 * d64 / to_nm + np.spacing(np.abs(f64))
    df = float((np.abs(fr.astype(np.float64) - f64.astype(np.float64)) / tol_f).max())
    print(f"{name}: d64 = {d64:.3e}; |dpos| = {dp:.3e}, |dvel| = {dv:.3e} ({max(dp, dv) / d64:.2f} d64; bar 100); frames {df:.3f} of their bar")
    out = os.environ.get("TI_MD_PARITY_OUT")
    if out:
        with open(out, "a") as fh:
            fh.write(f"{name}: B = {B}, {run['n_steps']} steps, dt = {run['dt'] * 1e3:g} fs, friction = {run['friction']:g} / ps: d64 = {d64:.3e}, "
                     f"|dpos| = {dp:.3e} nm, |dvel| = {dv:.3e} nm/ps, largest ratio to d64 = {max(dp, dv) / d64:.2f} (bar 100)\n")
    assert max(dp, dv) <= 100 * d64, (name, dp, dv, d64)
    assert df <= 1.0, (name, df)
    # the frame energies.  Potential: the energy tests' bar plus what 100 d64 of position error moves it, |dE| <= sum |F| |dx|, with
    # sum_a S^F_a >= sum |F|.  Kinetic: |dK| <= sum m |v| |dv| <= sqrt(3A m_max 2K) 100 d64, plus the arithmetic's 1e-11 (1 + K).
    for k in range(n_frames):
        _, SF, _ = ffn.forces(f64[:, k], to_nm, ff)
        Sb = fn.energies(f64[:, k], to_nm, ff)[2].sum(axis=1)
        assert (np.abs(ep[:, k] - e64[:, k]) <= 1e-11 * Sb + 100 * d64 * np.sqrt(3.0) * SF.sum(axis=1)).all(), (name, k)
    assert (np.abs(ek - k64) <= 1e-11 * (1 + k64) + 100 * d64 * np.sqrt(3 * len(m) * m.max() * 2 * k64)).all(), name
    assert np.abs(fr.astype(np.float64).mean(axis=2)).max() <= 2e-7 * np.abs(fr).max()          # centred to fp32 round-off
    return max(dp, dv) / d64


@pytest.mark.parametrize("name", ["A4", "A9"])
def test_trajectory_parity(name):
    if np.finfo(LD).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than float64 here: d64 cannot be formed")
    eng, ff, m, pos, T, ids, to_nm = case(name)
    check_trajectory(name, eng, ff, m, pos, T, ids, to_nm)


# ---- bits ------------------------------------------------------------------------------------------------------------------------
def run(eng, pos, vel, T, ids, to_nm, **over):
    kw = dict(RUN, **over)
    return eng.langevin(pos, vel, T, kw["dt"], kw["friction"], kw["n_steps"], stride=kw["stride"], seed=kw["seed"], ids=ids, to_nm=to_nm,
                        draw_velocities=vel is None, step_offset=kw.get("step_offset", 0), steps_per_launch=kw.get("steps_per_launch", 0),
                        traj_offset=kw.get("traj_offset", 0))


def same(a, b):
    for u, w in zip(a, b):
        np.testing.assert_array_equal(bits(u), bits(w))


def check_bits(eng, pos, T, ids, to_nm, strides=(4, 5, 3, 16, 17), **base):
    """the bitwise contract of one 16-step run (RUN with `base` over it): repeat, device memory, alone, reversed, ids NULL, chained,
    launch cut, strides"""
    import torch
    go = lambda *a, **over: run(eng, *a, **dict(base, **over))
    ref = go(pos, None, T, ids, to_nm)
    assert all(np.isfinite(a).all() for a in ref)
    same(go(pos, None, T, ids, to_nm), ref)                                                      # the same call twice
    dev = go(torch.from_numpy(pos).cuda(), None, torch.from_numpy(T).cuda(), torch.from_numpy(ids).cuda(), to_nm)
    assert all(a.is_cuda for a in dev) and dev[0].dtype == torch.float64 and dev[2].dtype == torch.float32
    same([a.cpu().numpy() for a in dev], ref)                                                    # device memory
    for b in (0, 3, 4):                                                                          # a replica alone, with its id
        same(go(pos[b:b + 1], None, T[b:b + 1], ids[b:b + 1], to_nm), [a[b:b + 1] for a in ref])
    rev = go(pos[::-1].copy(), None, T[::-1].copy(), ids[::-1].copy(), to_nm)                    # reversed batch, reversed ids
    same([a[::-1] for a in rev], ref)
    off = go(pos, None, T, None, to_nm, traj_offset=int(ids[0]))                                 # ids NULL: traj_offset + b
    same([a[:1] for a in off], [a[:1] for a in ref])
    # 16 steps against 8 + 8 chained with step_offset (given velocities, so that only the first call draws), frames included
    p0, v0, _, _, _ = go(pos, None, T, ids, to_nm, n_steps=0, stride=0)
    whole = go(p0, v0, T, ids, to_nm, step_offset=100)
    a = go(p0, v0, T, ids, to_nm, n_steps=8, step_offset=100)
    b = go(a[0], a[1], T, ids, to_nm, n_steps=8, step_offset=108)
    same(b[:2], whole[:2])
    same([np.concatenate([u, w], axis=1) for u, w in zip(a[2:], b[2:])], whole[2:])
    same(go(pos, None, T, ids, to_nm, steps_per_launch=5), ref)                                  # launches of 5, 5, 5, 1
    same(go(pos, None, T, ids, to_nm, steps_per_launch=16), ref)
    # strides that do not divide n_steps: the frames are those of the stride-1 run at the same steps
    every = go(pos, None, T, ids, to_nm, stride=1)
    same(every[:2], ref[:2])
    for stride in strides:
        got = go(pos, None, T, ids, to_nm, stride=stride, steps_per_launch=7)
        n = 16 // stride
        if n == 0:
            assert got[2] is None and got[3] is None
            continue
        assert got[2].shape[1] == n
        same(got[2:], [a[:, stride - 1::stride][:, :n] for a in every[2:]])


def test_bitwise_contract():
    pytest.importorskip("torch")
    eng, ff, m, pos, T, ids, to_nm = case("A9")
    assert int(ids[0]) == 7
    check_bits(eng, pos, T, ids, to_nm)


# ---- NVE -------------------------------------------------------------------------------------------------------------------------
def test_energy_conservation_without_a_thermostat():
    """A9, B = 3, friction = 0, dt = 0.25 fs, 2000 steps: the excursion of epot + ekin from its first frame against the restatement's
    own over the same run (leapfrog makes it a property of the scheme); the bar is twice the restatement's"""
    eng, ff, m, pos, T, ids, to_nm = case("A9", 3)
    vel = ffn.draw_velocities(T, ids, m, 5, 0)
    _, _, _, e_np, k_np = ffn.langevin(pos, vel, T, ids, ff, m, 2.5e-4, 0.0, 2000, stride=20, to_nm=to_nm, normal=None)
    p, v, _, ep, ek = eng.langevin(pos, vel, T, 2.5e-4, 0.0, 2000, stride=20, ids=ids, to_nm=to_nm, frames=False)
    tot, tot_np = ep + ek, e_np + k_np
    fl, fl_np = np.abs(tot - tot[:, :1]).max(axis=1), np.abs(tot_np - tot_np[:, :1]).max(axis=1)
    print(f"NVE: max |E - E0| GPU {fl}, numpy {fl_np}, E0 {tot[:, 0]}")
    assert ep.shape == (3, 100) and np.isfinite(tot).all() and (fl <= 2 * fl_np).all()
    np.testing.assert_allclose(tot[:, 0], tot_np[:, 0], rtol=1e-9)                              # the same run: its first frame agrees


# ---- physics ---------------------------------------------------------------------------------------------------------------------
def test_bond_length_distribution_of_a_diatomic():
    """A2: one bond, no live pair, masses 12.  256 replicas alternating 300 / 1000 K, dt = 1 fs, friction = 5 / ps, 2000 steps of
    equilibration, then 20000 steps with a frame every 20.  <r> and <(r - r0)^2> per temperature against the quadrature of
    r^2 exp(-k (r - r0)^2 / (2 R T)), within 5 standard errors of the 128 independent replica means (tests/test_adw_physics.py's bar)."""
    ti = pkg()
    eng, ff, m, x, to_nm = with_md("A2", masses=np.array([12.0, 12.0]))
    r0, k = ff["bond_par"][0]
    B = 256
    T = np.where(np.arange(B) % 2, 1000.0, 300.0).astype(np.float32)
    start = np.tile(np.array([[0.0, 0.0, 0.0], [r0, 0.0, 0.0]]), (B, 1, 1)) / to_nm
    smp = ti.md.LangevinSampler(eng, ti.forcefield.ForceField(**ff, masses=[12.0, 12.0]), to_nm, 1e-3, 5.0, seed=2024)
    smp.start(start, T).equilibrate(2000)
    frames, epot, ekin = smp.sample(1000, 20)
    assert frames.shape == (B, 1000, 2, 3) and smp.step == 22000
    r = np.linalg.norm((frames[:, :, 1] - frames[:, :, 0]).astype(np.float64), axis=-1) * to_nm
    grid = np.linspace(max(r0 - 0.08, 1e-4), r0 + 0.08, 200001)
    for temp in (300.0, 1000.0):
        w = grid ** 2 * np.exp(-k * (grid - r0) ** 2 / (2 * fn.R_GAS * temp))
        mean_q, var_q = (w * grid).sum() / w.sum(), (w * (grid - r0) ** 2).sum() / w.sum()
        rr = r[T == temp]
        for what, per_replica, want in (("<r>", rr.mean(axis=1), mean_q), ("<(r - r0)^2>", ((rr - r0) ** 2).mean(axis=1), var_q)):
            est, se = per_replica.mean(), per_replica.std(ddof=1) / np.sqrt(len(per_replica))
            z = (est - want) / se
            print(f"T = {temp:.0f} K {what}: {est:.6e} against {want:.6e}, z = {z:+.2f}, relative standard error {se / want:.2e}")
            assert abs(z) <= 5.0, (temp, what, z)
        # equipartition of the kinetic energy (6 degrees of freedom): sum m v^2 / 2 = 3 R T, a looser look at the thermostat
        kin = ekin[T == temp].mean(axis=1)
        zk = (kin.mean() - 3 * fn.R_GAS * temp) / (kin.std(ddof=1) / np.sqrt(len(kin)))
        print(f"T = {temp:.0f} K <ekin> = {kin.mean():.4f} against {3 * fn.R_GAS * temp:.4f}, z = {zk:+.2f}")


# ---- failure and refusals --------------------------------------------------------------------------------------------------------
def raw(eng, pos, vel, T, B=None, mem=0, ids=None, to_nm=1.0, frames=True, **d):
    """ti_obs_ff_langevin through ctypes on host memory with poisoned outputs -> (rc, frames, epot, ekin)"""
    ti = pkg()
    kw = dict(dt=5e-4, friction=1.0, n_steps=4, stride=2, step_offset=0, traj_offset=0, seed=1, draw_velocities=0, steps_per_launch=0)
    kw.update(d)
    desc = ti._lib.MdDesc(*(kw[k] for k in ("dt", "friction", "n_steps", "stride", "step_offset", "traj_offset", "seed", "draw_velocities",
                                           "steps_per_launch")))
    n = pos.shape[0] if pos is not None else 2
    A = 9 if pos is None else pos.shape[1]
    fr, ep, ek = np.full((n, 2, A, 3), -7.0, np.float32), np.full((n, 2), -7.0), np.full((n, 2), -7.0)
    ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    rc = ti._lib.lib().ti_obs_ff_langevin(eng.h, C.byref(desc) if d.get("desc", 1) else None, ptr(pos), ptr(vel), ptr(T), ptr(ids),
                                          n if B is None else B, to_nm, ptr(fr) if frames else None, ptr(ep) if frames else None,
                                          ptr(ek) if frames else None, mem)
    return rc, fr, ep, ek


def test_a_blown_up_replica_is_named_and_the_state_is_left_alone():
    """Two Lennard-Jones atoms 1e-4 nm apart at dt = 2 fs: the first step throws them some 1e40 nm apart, and the angle at the one that
    has two neighbours then has a cosine of exactly 1, whose force is 0 / 0.  The restatement says in which step the state stops being
    finite, so in which launch of one step each."""
    ti = pkg()
    eng, ff, m, pos, T, ids, to_nm = case("A9")
    tab = fn.pair_table(ff, 9)
    deg = np.bincount(np.asarray(ff["bond_idx"]).reshape(-1), minlength=9)
    i, j = next((i, j) for i in range(9) for j in range(9) if i != j and deg[i] >= 2 and tab[fn.pair_row(min(i, j), max(i, j), 9), 2] > 0)
    bad = pos.copy()
    bad[3, j] = bad[3, i] + np.array([1e-4, 0.0, 0.0])
    vel = np.zeros_like(bad)
    p_in, v_in = bad.copy(), vel.copy()
    p, v, first = bad[3:4], vel[3:4], None
    for s in range(9):
        p, v, _, _, _ = ffn.langevin(p, v, T[3:4], ids[3:4], ff, m, 2e-3, 0.0, 1, normal=None)
        if not (np.isfinite(p).all() and np.isfinite(v).all()):
            first = s
            break
    assert first is not None and first > 0                                                       # not in the first step: a later launch is named
    assert first == 1
    rc, fr, ep, ek = raw(eng, bad, vel, T, dt=2e-3, friction=0.0, n_steps=9, stride=5, steps_per_launch=1)
    assert rc == ti._lib.TI_E_NAN and "replica 3" in ti._lib.last_error() and f"launch {first} " in ti._lib.last_error(), ti._lib.last_error()
    np.testing.assert_array_equal(bits(bad), bits(p_in)); np.testing.assert_array_equal(bits(vel), bits(v_in))
    assert (fr == -7.0).all() and (ep == -7.0).all() and (ek == -7.0).all()                     # a host call copies nothing back
    with pytest.raises(ti._lib.TiError, match="replica 3"):
        eng.langevin(bad, vel, T, 2e-3, 0.0, 9, stride=5, to_nm=1.0)
    rc, _, _, _ = raw(eng, pos.copy(), np.zeros_like(pos), T)                                    # the handle goes on working
    assert rc == 0


def test_refusals_leave_everything_untouched():
    ti = pkg()
    L, ARG, UNS = ti._lib.lib(), ti._lib.TI_E_ARG, ti._lib.TI_E_UNSUPPORTED
    eng, ff, m, pos, T, ids, to_nm = case("A9")
    vel = np.zeros_like(pos)
    p_in = pos.copy()

    def refused(code, rc_fr, what):
        rc, fr, ep, ek = rc_fr
        assert rc == code and ti._lib.last_error(), what
        assert (fr == -7.0).all() and (ep == -7.0).all() and (ek == -7.0).all(), what
        np.testing.assert_array_equal(bits(pos), bits(p_in), err_msg=what)
        assert (vel == 0).all(), what

    refused(ARG, raw(eng, pos, vel, T, desc=0), "NULL desc")
    refused(ARG, raw(eng, None, vel, T), "NULL pos")
    refused(ARG, raw(eng, pos, vel, None), "NULL T")
    refused(ARG, raw(eng, pos, None, T), "NULL vel without draw_velocities")
    for dt in (0.0, -1e-3, np.nan, np.inf):
        refused(ARG, raw(eng, pos, vel, T, dt=dt), f"dt = {dt}")
    refused(ARG, raw(eng, pos, vel, T, friction=-1.0), "friction < 0")
    refused(ARG, raw(eng, pos, vel, T, n_steps=-1), "n_steps < 0")
    refused(ARG, raw(eng, pos, vel, T, stride=-1), "stride < 0")
    refused(ARG, raw(eng, pos, vel, T, frames=False), "stride > 0 with every output NULL")
    refused(ARG, raw(eng, pos, vel, T, B=0), "B < 1")
    refused(ARG, raw(eng, pos, vel, T, mem=7), "unknown mem")
    for value in (0.0, -300.0, np.nan, np.inf):                                                  # found on the device, nothing written
        Tb = np.full(5, 300.0, np.float32)
        Tb[2], Tb[4] = value, value
        refused(ARG, raw(eng, pos, vel, Tb), f"T = {value}")
        assert "index 2" in ti._lib.last_error()
    adw = ti.observables._service_engine(0)
    refused(ARG, raw(adw, pos, vel, T), "an adw handle")
    eng.set_molecules(np.full(5, 9, np.int32))
    try:
        refused(UNS, raw(eng, pos, vel, T), "ti_painn_set_molecules in force")
    finally:
        eng.set_molecules(None)
    # masses: a bad one is refused and the ones in force stay; cleared with the force field
    good = raw(eng, pos.copy(), vel.copy(), T)
    assert good[0] == 0
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    for value in (0.0, -1.0, np.nan, np.inf):
        mb = m.copy()
        mb[4] = value
        assert L.ti_obs_ff_set_masses(eng.h, dp(mb)) == ARG and "mass 4" in ti._lib.last_error()
        again = raw(eng, pos.copy(), vel.copy(), T)
        assert again[0] == 0 and all(np.array_equal(bits(u), bits(w)) for u, w in zip(again[1:], good[1:]))
    eng.set_forcefield(ti.forcefield.ForceField(**ff))                                           # a force field without masses
    refused(ARG, raw(eng, pos, vel, T), "no masses")
    assert "masses" in ti._lib.last_error()
    with pytest.raises(ValueError, match="masses"):
        eng.langevin(pos, vel, T, 5e-4, 1.0, 4)
    zero = m.copy()
    zero[0] = 0.0
    eng.set_forcefield(ti.forcefield.ForceField(**ff, masses=zero))
    with pytest.raises(ValueError, match="masses"):
        eng.langevin(pos, vel, T, 5e-4, 1.0, 4)
    eng.set_forcefield(ti.forcefield.ForceField(**ff, masses=m, has_constraints=True))
    with pytest.raises(ValueError, match="constraints"):
        eng.langevin(pos, vel, T, 5e-4, 1.0, 4)
    assert np.isfinite(eng.ff_energy(pos.astype(np.float32), 1.0)).all()                         # the energies do not mind them
    eng.set_forcefield(None)
    refused(ARG, raw(eng, pos, vel, T), "no force field")


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def test_generate_md_end_to_end(tmp_path):
    ti = pkg()
    ff, m, x, to_nm = species("A4")
    write_xml(ff, tmp_path / "ff.xml")
    text = (tmp_path / "ff.xml").read_text()
    for a in range(4):                                                                           # the species' masses in place of the writer's 1
        text = text.replace('<Particle mass="1"/>', f'<Particle mass="{float(m[a])!r}"/>', 1)
    (tmp_path / "ff.xml").write_text(text)
    np.save(tmp_path / "x0.npy", x[:3].astype(np.float64))
    cfg = types.SimpleNamespace(forcefield=str(tmp_path / "ff.xml"), x0=str(tmp_path / "x0.npy"), to_nm=to_nm, temperatures=[300, 1000],
                                n_replicas=4, dt=5e-4, friction=1.0, n_equil=10, n_frames=8, stride=2, seed=3,
                                splits={"train": 0.5, "val": 0.25, "test": 0.25}, traj_path=str(tmp_path / "md"), traj_filename="mol.npy")
    paths = ti.drivers.generate_md(cfg, engine(4))
    for split, n in (("train", 2), ("val", 1), ("test", 1)):
        a = np.load(paths[split])
        assert a.shape == (8, n * 8, 4, 3) and a.dtype == np.float32 and np.isnan(a[1:7]).all() and np.isfinite(a[[0, 7]]).all()
        assert np.abs(a[[0, 7]].astype(np.float64).mean(axis=2)).max() <= 2e-7 * np.abs(a[[0, 7]]).max()      # centred to fp32 round-off
        got = ti.data.load_trajectory(cfg.traj_path, split, "mol.npy", 300, scale=False)
        assert got.shape == (n * 8, 4, 3) and np.abs(got - a[0]).max() <= 4e-7 * np.abs(a[0]).max()
    with np.load(os.path.join(cfg.traj_path, "md_log.npz")) as z:
        assert z["epot"].shape == (2, 4, 8) and np.isfinite(z["epot"]).all() and np.isfinite(z["ekin"]).all()
    # the first train frame of 300 K is the run's: replica 0, step 12 of a run that the sampler makes the same way
    smp = ti.md.LangevinSampler(engine(4), ti.forcefield.ForceField.from_openmm_xml(cfg.forcefield), to_nm, 5e-4, 1.0, 3)
    smp.start(x[np.arange(8) % 3].astype(np.float64), np.repeat(np.float32([300, 1000]), 4)).equilibrate(10)
    fr, _, _ = smp.sample(8, 2)
    np.testing.assert_array_equal(bits(np.load(paths["train"])[0, :8]), bits(fr[0]))
