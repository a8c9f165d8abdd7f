"""CPU: the option surface of per-trajectory dopri5 step control and of per-molecule drift times -- validation that happens
before any device is touched (no GPU needed)."""
import ctypes as C
import types

import numpy as np
import pytest

from conftest import pkg


@pytest.fixture(scope="module")
def lib():
    ti = pkg()
    ti.build.build()
    return ti._lib.lib()


def test_step_control_is_validated_in_every_layer():
    ti = pkg()
    amb, lat, adw = ti.thermo.ambient, ti.thermo.latent, ti.thermo.adw
    b = amb.cPaiNN(n_features=32, score_layers=2, temp_length=100)
    for cls in (amb.MoleculeIntegrator, lat.MoleculeIntegrator):
        assert cls(b=b, n_step=10).step_control == "batch"                       # default: today's behaviour
        assert cls(b=b, n_step=10, step_control="trajectory").step_control == "trajectory"
        assert cls(b=b, n_step=10, return_dlogp=True, step_control="trajectory").method == "dopri5"
        for method in ("euler", "heun", "midpoint", "rk4", "em"):
            with pytest.raises(ValueError, match="dopri5"):
                cls(b=b, method=method, n_step=10, step_control="trajectory")
        with pytest.raises(ValueError, match="step_control"):
            cls(b=b, n_step=10, step_control="molecule")
        with pytest.raises(TypeError):                                           # keyword-only
            cls(b, "dopri5", 10, 1e-4, 1e-4, 0.0, 1.0, False, False, "trajectory")
    net = adw.FCNetMultiBeta(1, 1, 64, 3)
    assert adw.StandardIntegrator(b=net, n_step=11, step_control="trajectory").step_control == "trajectory"
    with pytest.raises(ValueError, match="dopri5"):
        adw.StandardIntegrator(b=net, method="rk4", n_step=11, step_control="trajectory")
    with pytest.raises(ValueError, match="step_control"):
        adw.StandardIntegrator(b=net, n_step=11, step_control="")
    # engine level: the scheme code of the C ABI
    assert ti.engine.scheme_code("dopri5") == 3
    assert ti.engine.scheme_code("dopri5", "trajectory") == 6
    with pytest.raises(ValueError, match="dopri5"):
        ti.engine.scheme_code("heun", "trajectory")
    with pytest.raises(ValueError, match="step_control"):
        ti.engine.scheme_code("dopri5", "per-molecule")


def test_per_molecule_times_are_checked_before_the_device():
    ti = pkg()
    mol = ti.thermo._molecule
    t = np.repeat(np.asarray([0.1, 0.5, 0.9], np.float32), 4)                 # per node, constant within each of 3 molecules
    np.testing.assert_array_equal(mol.molecule_times(t, 3, 4), np.asarray([0.1, 0.5, 0.9], np.float32))
    assert mol.molecule_times(np.full(12, 0.25, np.float32), 3, 4) == 0.25     # uniform: the scalar-t path
    assert mol.molecule_times(np.float32(0.75), 3, 4) == 0.75
    bad = t.copy()
    bad[5] = 0.6                                                              # varies inside molecule 1
    with pytest.raises(ValueError, match="constant within each molecule"):
        mol.molecule_times(bad, 3, 4)
    with pytest.raises(ValueError):
        mol.molecule_times(np.arange(5, dtype=np.float32), 3, 4)
    # cPaiNN.forward refuses a time that varies inside a molecule before it creates an engine
    syn = ti.synthetic
    A, B = 4, 3
    src, dst, ety = syn.fully_connected_template(A)
    batch = types.SimpleNamespace(x=syn.molecule_coords(B, A, 0).reshape(B * A, 3), atoms=np.tile(np.arange(A), B),
                                  edge_index=syn.batch_edge_index(src, dst, A, B), edge_type=np.tile(ety, B),
                                  batch=np.repeat(np.arange(B), A), T0=np.full(B * A, 300.0), T1=np.full(B * A, 400.0), t=bad)
    b = ti.thermo.ambient.cPaiNN(n_features=32, score_layers=2, temp_length=100)
    with pytest.raises(ValueError, match="constant within each molecule"):
        b.forward(batch)
    with pytest.raises(ValueError, match="constant within each molecule"):
        ti.thermo.ambient.ODEWrapper.compute_divergence(b, batch)
    net = ti.thermo.adw.FCNetMultiBeta(1, 1, 64, 3)
    with pytest.raises(ValueError, match="one per row"):
        net.forward(None, np.zeros((4, 1)), np.asarray([[0.1], [0.2]]), np.ones((4, 1)), np.ones((4, 1)))


def test_new_abi_entries_refuse_null_arguments(lib):
    ti = pkg()
    E = ti._lib.TI_E_ARG
    f = C.c_void_p(0)
    assert lib.ti_painn_drift_tv(None, None, None, None, 1, None, 0) == E
    assert lib.ti_painn_drift_div_tv(None, None, None, None, 1, None, None, 0) == E
    assert lib.ti_adw_drift_tv(None, None, None, None, None, 1, None, None, 0) == E
    acc, rej = np.zeros(2, np.int64), np.zeros(2, np.int64)
    p = C.POINTER(C.c_int64)
    assert lib.ti_rollout_step_counts(None, acc.ctypes.data_as(p), rej.ctypes.data_as(p), 2) == E
    assert lib.ti_rollout_step_counts(f, None, None, 2) == E
    assert "NULL" in lib.ti_last_error().decode()


def test_rollout_desc_accepts_scheme_6_and_refuses_7(lib):
    ti = pkg()
    grid = np.linspace(0, 1, 3).astype(np.float32)
    rd = ti.engine._rollout_desc("dopri5", grid, 1, 0, 0.0, 0, 0, False, 1e-4, 1e-4, step_control="trajectory")
    assert rd.scheme == 6
    # the descriptor is checked before the handle: scheme 6 passes and the call stops at the missing handle
    assert lib.ti_painn_rollout(None, C.byref(rd), None, None, 1, None, None) == ti._lib.TI_E_ARG
    assert "painn handle" in lib.ti_last_error().decode()
    rd.scheme = 7
    assert lib.ti_painn_rollout(None, C.byref(rd), None, None, 1, None, None) == ti._lib.TI_E_ARG
    assert "unknown scheme" in lib.ti_last_error().decode()
    rd.scheme, rd.rtol = 6, 0.0                                               # same tolerance rules as dopri5
    assert lib.ti_painn_rollout(None, C.byref(rd), None, None, 1, None, None) == ti._lib.TI_E_ARG
    assert "rtol" in lib.ti_last_error().decode()


@pytest.mark.parametrize("name", ["tv_ambient", "tv_latent_multi"])
def test_per_molecule_time_fixtures_match_the_oracle_row_by_row(name):
    """The tv_* fixtures (reference cPaiNN at one batch.t per molecule) equal, molecule by molecule, the CPU oracle's scalar-t drift
    at that molecule's time: what the per-molecule entry points must reproduce."""
    from conftest import golden_weights, load_golden, rel_l2
    from oracle import oracle
    g = load_golden(name)
    args = (int(g["variant"]), int(g["F"]), int(g["L"]), int(g["A"]), g["edge_src"], g["edge_dst"], g["edge_type"], g["atom_ids"], golden_weights(g))
    orc = oracle.PainnOracle(*args, temp_length=float(g["temp_length"]), temperatures=g["temperatures"])
    assert len(set(g["tv"].tolist())) == int(g["B"])
    for b in range(int(g["B"])):
        assert rel_l2(orc.drift(g["x"], float(g["tv"][b]), g["cond"])[b], g["drift_tv"][b]) < 1e-5
