"""Observables without a GPU: the fp64 restatement (tests/obs_numpy.py) against the reference's own geometry functions and ESS
(tests/golden/obs_geometry.npz, written by tests/golden/make_golden_obs.py), the C ABI (declared, exported, listed, refusals that
come before any device work), the argument checks of observables.py, the driver's file set without the `observables` key, and the
code objects of the new kernels (no private segment, no spills)."""
import os
import re
import tempfile
import types

import numpy as np
import pytest

from conftest import ROOT, load_golden, pkg
import obs_numpy as on
import test_build_isa as isa_rules
from test_edge_mask_host import _kernel_metadata

NEW_SYMBOLS = ("ti_obs_cv", "ti_obs_weights", "ti_obs_hist", "ti_obs_set_observer")
NEW_KERNELS = ("obs_cv_kernel", "obs_logw_max_kernel", "obs_logw_kernel", "obs_combine_kernel", "obs_weights_kernel", "obs_whist_kernel")


# ------------------------------------------------------------------------------------------------------------ the oracle
def test_restatement_reproduces_the_reference_fixture():
    """1e-6 absolute: the reference computes in fp32, the restatement in fp64 from the same fp32 coordinates."""
    g = load_golden("obs_geometry")
    x = g["x"]
    assert x.shape == (7, 9, 3) and x.dtype == np.float32
    for name in ("dist", "angle", "torsion"):
        assert np.isfinite(g[name]).all(), name
    at = lambda idx: [x[:, i] for i in idx]
    for k, t in enumerate(g["dist_idx"]):
        assert np.abs(on.distance(*at(t)) - g["dist"][:, k]).max() < 1e-6, t
    for k, t in enumerate(g["angle_idx"]):
        assert np.abs(on.angle(*at(t)) - g["angle"][:, k]).max() < 1e-6, t
    for k, t in enumerate(g["torsion_idx"]):
        assert np.abs(on.torsion(*at(t)) - g["torsion"][:, k]).max() < 1e-6, t
    # the cases the fixture is there for: torsions near 0, +pi and -pi, an angle near pi
    t0 = g["torsion"][:3, 0]
    assert abs(t0[0]) < 0.05 and t0[1] > np.pi - 0.05 and t0[2] < -np.pi + 0.05
    assert g["angle"][3, 2] > np.pi - 0.3
    w, ess = on.importance_weights(np.log(g["weights"]))
    assert abs(ess - float(g["ess"])) < 1e-9 * float(g["ess"])
    assert abs(w.sum() - 1.0) < 1e-12
    # the same through collective_variables, mixing the kinds
    desc = np.array([[on.DIST, *g["dist_idx"][0], 0, 0], [on.ANGLE, *g["angle_idx"][2], 0], [on.TORSION, *g["torsion_idx"][0]]], np.int32)
    cv = on.collective_variables(x, desc)
    assert np.abs(cv - np.stack([g["dist"][:, 0], g["angle"][:, 2], g["torsion"][:, 0]], axis=1)).max() < 1e-6


def test_restated_rmsd_keeps_reflections_out_and_histogram_edge_rules():
    rs = np.random.RandomState(0)
    ref = rs.standard_normal((9, 3))
    q, _ = np.linalg.qr(rs.standard_normal((3, 3)))
    q *= np.sign(np.linalg.det(q))
    assert on.kabsch_rmsd((ref @ q.T + 3.0)[None], ref)[0] < 1e-7
    assert on.kabsch_rmsd((ref * [1, 1, -1])[None], ref)[0] > 0.1            # the mirror image of a chiral frame
    sel = np.array([1, 1, 0, 1, 0, 1, 1, 1, 0])
    moved = ref.copy()
    moved[sel == 0] += 5.0
    assert on.kabsch_rmsd(moved[None], ref, sel)[0] < 1e-7
    v = np.array([-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 3.0, np.nan, np.inf], np.float32)
    hist, tails = on.weighted_histogram(v, None, 4, 0.0, 2.0)
    np.testing.assert_allclose(hist * 9, [1, 1, 1, 1])                         # lo -> bin 0; interior edges go up
    np.testing.assert_allclose(tails * 9, [1, 2, 2])                           # below; hi itself and above; NaN and inf
    f = on.free_energy_profile(np.array([0.1, 0.1, 0.6], np.float32), None, 4, 0.0, 2.0)
    np.testing.assert_allclose(f[:2], -np.log(np.array([2 / 3, 1 / 3]) / 0.5))
    assert np.isinf(f[2:]).all()


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_symbols_declared_exported_and_listed():
    ti = pkg()
    hdr = open(os.path.join(ROOT, "include", "ti_hip.h")).read()
    L = ti._lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(ti_handle\* h, ", hdr), name
        assert name in ti._lib.ABI_SYMBOLS and hasattr(L, name), name
    assert "TI_SCHEME_DOPRI5_TRAJ writes its rows per trajectory inside a" in hdr and "TI_E_UNSUPPORTED" in hdr
    assert L.ti_version() == 5


def test_refusals_before_the_device():
    ti = pkg()
    L = ti._lib.lib()
    E = ti._lib.TI_E_ARG
    assert L.ti_obs_cv(None, None, 1, None, None, None, 1, None, 0) == E
    assert L.ti_obs_weights(None, None, 1, None, None, 0) == E
    assert L.ti_obs_hist(None, None, 1, None, 1, 4, 0.0, 1.0, None, None, 0) == E
    assert L.ti_obs_set_observer(None, None, 0, None, None, 1, None, 0) == E
    assert ti._lib.last_error() == "NULL handle"


def test_python_argument_validation():
    ti = pkg()
    obs = ti.observables
    d = obs.encode_descriptors([("rmsd",), ("dist", 0, 1), ("angle", 0, 1, 2), ("torsion", 3, 2, 1, 0), "rmsd"])
    np.testing.assert_array_equal(d, [[0, 0, 0, 0, 0], [1, 0, 1, 0, 0], [2, 0, 1, 2, 0], [3, 3, 2, 1, 0], [0, 0, 0, 0, 0]])
    np.testing.assert_array_equal(obs.encode_descriptors(d), d)
    np.testing.assert_array_equal(obs.encode_descriptors([("coord", 2)]), [[4, 2, 0, 0, 0]])
    for bad, msg in (([], "at least one"), ([("bond", 0, 1)], "unknown kind"), ([("dist", 0)], "takes 2"), ([("torsion", 0, 1, 2)], "takes 4"),
                     ([("rmsd", 1)], "takes 0"), ([("dist", 0, -1)], "negative")):
        with pytest.raises(ValueError, match=msg):
            obs.encode_descriptors(bad)
    for bins, rng in ((0, (0, 1)), (257, (0, 1)), (2.5, (0, 1)), (8, (1, 1)), (8, (2, 1)), (8, (0, np.inf))):
        with pytest.raises(ValueError):
            obs.check_bins(bins, rng)
    assert obs.check_bins(80, (-2.5, 2.5)) == (80, -2.5, 2.5)
    assert obs.check_observe(None) is None
    o = obs.check_observe(dict(descriptors=[("rmsd",)], ref=np.zeros((3, 3))))
    assert o["every"] == 1 and o["select"] is None
    for bad in ("rmsd", dict(ref=None), dict(descriptors=[("rmsd",)], evry=2), dict(descriptors=[("rmsd",)], every=-1)):
        with pytest.raises(ValueError):
            obs.check_observe(bad)
    with pytest.raises(ValueError, match="trajectory"):
        ti.thermo.adw.StandardIntegrator(None, method="dopri5", step_control="trajectory", observe=dict(descriptors=[("coord", 0)]))
    # engine-side shape checks come before the library
    eng = ti.engine.PainnEngine.__new__(ti.engine.PainnEngine)
    eng.A, eng.h = 4, None
    with pytest.raises(ValueError, match="ref must be"):
        eng.collective_variables(np.zeros((2, 4, 3), np.float32), [("rmsd",)], ref=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="select must be"):
        eng.collective_variables(np.zeros((2, 4, 3), np.float32), [("rmsd",)], ref=np.zeros((4, 3)), select=[1, 0])
    with pytest.raises(ValueError, match="1-D"):
        eng.weighted_histogram(np.zeros((4, 2), np.float32), None, 8, (0, 1))
    with pytest.raises(ValueError, match="bins"):
        eng.weighted_histogram(np.zeros(4, np.float32), None, 300, (0, 1))
    f = ti.observables.profile_from_histogram([0.5, 0.0, 0.25, 0.25], 0.0, 2.0)
    np.testing.assert_allclose(f[[0, 2, 3]], -np.log(np.array([0.5, 0.25, 0.25]) / 0.5))
    assert np.isinf(f[1])


def test_driver_without_the_key_writes_todays_files(tmp_path, monkeypatch):
    """sample_adw with a stand-in rollout (no GPU): the file set is exactly the reference's three files."""
    ti = pkg()
    n_step, seen = 5, {}

    def rollout(self, x0s, beta0s, beta1s, traj_offset=0):
        seen["observe"] = self.observe
        B = x0s.shape[0]
        return np.zeros((n_step, B, 1), np.float32), np.zeros((n_step, B, 1), np.float32)

    monkeypatch.setattr(ti.thermo.adw.StandardIntegrator, "rollout", rollout)
    net = types.SimpleNamespace(dim=1, eval=lambda: None)
    cfg = types.SimpleNamespace(beta0s=[1.0], beta1s=[1.25], solver_type="euler", rtol=1e-4, atol=1e-4, n_step=n_step, return_dlogp=1,
                                data_save_path=str(tmp_path), model_save_name="m", sampling_epoch=2)
    loader = [(np.zeros((4, 1), np.float32), np.ones((4, 1)))]
    ti.drivers.sample_adw(cfg, net, loader)
    assert seen["observe"] is None
    out_dir = tmp_path / "m" / "beta_1.0_to_1.25"
    assert sorted(os.listdir(out_dir)) == ["dlogps_epoch_2.npy", "initial_samples_epoch_2.npy", "samples_epoch_2.npy"]
    assert ti.drivers._observe_kw(cfg) == {}
    cfg.observables = {"descriptors": [["coord", 0]], "every": 2, "bins": 16}
    kw = ti.drivers._observe_kw(cfg)["observe"]
    assert kw == {"descriptors": [["coord", 0]], "every": 2}


# ------------------------------------------------------------------------------------------------------------ code objects
@pytest.fixture(scope="module")
def code_objects():
    tools = [isa_rules._tool(t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump")]
    if not all(tools):
        pytest.skip("ROCm LLVM tools not found")
    if not os.path.exists(isa_rules.LIB):
        pytest.skip(f"{isa_rules.LIB} not built")
    tmp = tempfile.TemporaryDirectory()
    yield isa_rules.code_objects(isa_rules.LIB, tmp.name)
    tmp.cleanup()


def test_new_kernels_exist_without_scratch_or_spills(code_objects):
    meta = {}
    for co in code_objects:
        meta.update(_kernel_metadata(co))
    for tag in NEW_KERNELS:
        hits = {n: m for n, m in meta.items() if f"{len(tag)}{tag}" in n}
        assert len(hits) == 1, (tag, sorted(hits))
        assert list(hits.values())[0] == (0, 0, 0), hits


def test_recorded_isa_comparison_with_the_parent_build():
    """tools/isa_compare.py PARENT.so THIS.so, recorded: no kernel of the parent differs or is missing; the added ones are the above."""
    text = open(os.path.join(ROOT, "profiles", "obs_isa_compare.txt")).read()
    m = re.search(r"(\d+) symbols in \S+; identical in \S+: (\d+); differing: (\d+); missing: (\d+); added: (\d+)", text)
    assert m, text[:400]
    total, same, diff, missing, added = map(int, m.groups())
    assert total == same and diff == 0 and missing == 0
    added_names = re.findall(r"^ADDED (.*)$", text, flags=re.M)
    assert added == len(added_names) == len(NEW_KERNELS)
    for tag in NEW_KERNELS:
        assert any(tag in n for n in added_names), tag
