"""GPU: every entry point of libti_hip.so that takes `mem` (directly, or through its rollout descriptor) gives the same bits for
host arrays (TI_MEM_HOST: inputs mirrored in the handle's buffers, outputs copied back) and for device tensors (TI_MEM_DEVICE:
pointers used as they are), and leaves its inputs alone.  The PaiNN handle is F = 32, L = 2, A = 5 fully connected with per-node
conditioning (ncond = 2) and B = 3, which leaves the last group of the throughput layout (G = 4) partial; the adw handles are
H = 32 with two layers, dim = 1 and dim = 2, B = 5 rows over two distinct (beta0, beta1) pairs."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import pkg

pytestmark = pytest.mark.gpu

F, L, A, B = 32, 2, 5, 3
BA = 5
GRID3 = np.linspace(0.0, 1.0, 3, dtype=np.float32)
TRAJ = dict(scheme="dopri5", step_control="trajectory")
EST = dict(n_probes=2, probe_seed=7, traj_offset=11)
CVS = [("dist", 0, 1), ("angle", 0, 1, 2), ("torsion", 0, 1, 2, 3), ("rmsd",)]


@functools.lru_cache(maxsize=None)
def engines():
    """name -> (engine, host inputs): built once, shared by every case."""
    ti = pkg()
    syn, W, E = ti.synthetic, ti.weights, ti.engine
    rs = np.random.RandomState(5)
    flat = W.flatten_state_dict(syn.painn_state_dict(W.AMBIENT, F, L, 25, 3), W.painn_param_spec(W.AMBIENT, F, L, 25))
    painn = E.PainnEngine(W.AMBIENT, F, L, A, *syn.fully_connected_template(A), np.arange(A), flat, temp_length=100.0)
    assert painn.ncond > 0
    painn.set_template("throughput")
    x = syn.molecule_coords(B, A, seed=2)
    out = {"painn": (painn, dict(x=x, cond=syn.ambient_cond(B, A), xdot=rs.randn(B, A, 3).astype(np.float32),
                                 tv=np.array([0.2, 0.5, 0.8], np.float32), ref=x[0].copy()))}
    for d in (1, 2):
        spec = W.adw_param_spec(32, 2, d, d)
        eng = E.AdwEngine(32, 2, W.flatten_state_dict(syn.make_state_dict(spec, seed=4 + d, dtype=np.float64), spec, dtype=np.float64), dim=d)
        out[f"adw{d}"] = (eng, dict(x=rs.randn(*eng._xs(BA)).astype(np.float32), tv=np.linspace(0.1, 0.9, BA, dtype=np.float32),
                                    b0=np.array([1.0, 1.0, 1.0, 2.0, 2.0], np.float32), b1=np.array([1.25, 1.25, 2.0, 2.0, 1.25], np.float32)))
    return out


# (id, engine, call(engine, inputs) -> tuple of outputs): `inputs` holds numpy arrays or CUDA tensors of the same values
CALLS = [
    ("painn_drift", "painn", lambda e, a: (e.drift(a.x, 0.3, a.cond),)),
    ("painn_drift_tv", "painn", lambda e, a: (e.drift(a.x, a.tv, a.cond),)),
    ("painn_drift_jvp", "painn", lambda e, a: e.jvp(a.x, a.xdot, 0.3, a.cond)),
    ("painn_drift_div", "painn", lambda e, a: e.drift_div(a.x, 0.3, a.cond)),
    ("painn_drift_div_tv", "painn", lambda e, a: e.drift_div(a.x, a.tv, a.cond)),
    ("painn_drift_div_est", "painn", lambda e, a: e.drift_div_est(a.x, 0.3, a.cond, **EST)),
    ("painn_drift_div_est_tv", "painn", lambda e, a: e.drift_div_est(a.x, a.tv, a.cond, **EST)),
    ("painn_rollout_heun", "painn", lambda e, a: e.rollout(a.x, a.cond, GRID3, scheme="heun")),
    ("painn_rollout_dopri5_traj", "painn", lambda e, a: e.rollout(a.x, a.cond, GRID3, **TRAJ)),
    ("painn_rollout_dlogp_heun", "painn", lambda e, a: e.rollout_dlogp(a.x, a.cond, GRID3, scheme="heun")),
    ("painn_rollout_dlogp_dopri5_traj", "painn", lambda e, a: e.rollout_dlogp(a.x, a.cond, GRID3, **TRAJ)),
    ("painn_rollout_dlogp_est", "painn", lambda e, a: e.rollout_dlogp_est(a.x, a.cond, GRID3, **EST)),
    ("painn_obs_cv", "painn", lambda e, a: (e.collective_variables(a.x, CVS, ref=a.ref),)),
]
for _d in (1, 2):
    CALLS += [
        (f"adw{_d}_drift", f"adw{_d}", lambda e, a: (e.drift(a.x, 0.3, a.b0, a.b1),)),
        (f"adw{_d}_drift_div", f"adw{_d}", lambda e, a: e.drift(a.x, 0.3, a.b0, a.b1, return_div=True)),
        (f"adw{_d}_drift_tv", f"adw{_d}", lambda e, a: e.drift(a.x, a.tv, a.b0, a.b1, return_div=True)),
        (f"adw{_d}_rollout", f"adw{_d}", lambda e, a: e.rollout(a.x, a.b0, a.b1, GRID3, scheme="heun")),
        (f"adw{_d}_rollout_dlogp", f"adw{_d}", lambda e, a: e.rollout(a.x, a.b0, a.b1, GRID3, scheme="heun", return_dlogp=True)),
        (f"adw{_d}_rollout_dlogp_dopri5_traj", f"adw{_d}", lambda e, a: e.rollout(a.x, a.b0, a.b1, GRID3, return_dlogp=True, **TRAJ)),
        (f"adw{_d}_obs_cv", f"adw{_d}", lambda e, a: (e.collective_variables(a.x, [("coord", 0)]),)),
    ]
CALLS += [("adw1_rollout_fused", "adw1", lambda e, a: e.rollout(a.x, a.b0, a.b1, GRID3, scheme="heun", return_dlogp=True, fused=True)),
          ("adw1_rollout_fused_em", "adw1", lambda e, a: e.rollout(a.x, a.b0, a.b1, GRID3, scheme="em", eps=0.01, seed=3, fused=True))]


def inputs_of(name, device):
    """Fresh copies of the inputs of engine `name`: numpy arrays, or CUDA tensors of the same values."""
    host = {k: v.copy() for k, v in engines()[name][1].items()}
    if not device:
        return SimpleNamespace(**host)
    import torch
    return SimpleNamespace(**{k: torch.from_numpy(v).cuda() for k, v in host.items()})


def to_numpy(v):
    return v.cpu().numpy() if hasattr(v, "data_ptr") else np.asarray(v)


@pytest.mark.parametrize("case", CALLS, ids=[c[0] for c in CALLS])
def test_host_and_device_paths_agree_bit_for_bit(case):
    pytest.importorskip("torch")
    _, name, call = case
    eng, original = engines()[name]
    got = []
    for device in (False, True):
        a = inputs_of(name, device)
        outs = call(eng, a)
        for k, v in original.items():                       # the inputs are the caller's: never written
            np.testing.assert_array_equal(to_numpy(getattr(a, k)), v, err_msg=f"{case[0]}: input {k} changed (device={device})")
        assert all(hasattr(o, "data_ptr") and o.is_cuda for o in outs if not isinstance(o, int)) == device
        got.append([to_numpy(o) for o in outs])
    assert len(got[0]) == len(got[1])
    for i, (h, d) in enumerate(zip(*got)):
        assert h.shape == d.shape and np.isfinite(h).all(), (case[0], i)
        np.testing.assert_array_equal(d, h, err_msg=f"{case[0]}: output {i}")


def test_debug_tap_leaves_the_host_output_untouched():
    """A debug tap stops ti_painn_drift after the tapped stage: with host buffers nothing is copied back into `out`."""
    eng, a = engines()["painn"]
    ref = eng.drift(a["x"], 0.3, a["cond"])
    out = np.full((B, A, 3), 7.0, np.float32)
    eng.debug_tap(1)
    try:
        eng.drift(a["x"], 0.3, a["cond"], out=out)
    finally:
        eng.debug_tap(-1)
    np.testing.assert_array_equal(out, np.full((B, A, 3), 7.0, np.float32))
    np.testing.assert_array_equal(eng.drift(a["x"], 0.3, a["cond"], out=out), ref)
