"""CPU: the option surface of Hutchinson's divergence estimator (include/ti_hip.h ti_painn_drift_div_est) -- keyword validation, the
defaults that keep the exact path, the drivers' config keys, and the C ABI declarations (no GPU needed)."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from conftest import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ti_painn_drift_div_est", "ti_painn_drift_div_est_tv", "ti_painn_rollout_dlogp_est")


@pytest.fixture(scope="module")
def lib():
    ti = pkg()
    ti.build.build()
    return ti._lib.lib()


def _integrators():
    ti = pkg()
    b = ti.thermo.ambient.cPaiNN(n_features=32, score_layers=2, temp_length=100)
    return b, (ti.thermo.ambient.MoleculeIntegrator, ti.thermo.latent.MoleculeIntegrator)


def test_defaults_keep_the_exact_divergence():
    b, classes = _integrators()
    for cls in classes:
        for dl in (False, True):
            integ = cls(b=b, n_step=10, return_dlogp=dl)
            assert integ.divergence == "exact" and integ.n_probes == 1 and integ.probe_seed == 0


def test_divergence_keywords_are_validated():
    b, classes = _integrators()
    for cls in classes:
        integ = cls(b=b, method="heun", n_step=10, return_dlogp=True, divergence="hutchinson", n_probes=4, probe_seed=7)
        assert (integ.divergence, integ.n_probes, integ.probe_seed) == ("hutchinson", 4, 7)
        assert cls(b=b, n_step=10, return_dlogp=True, divergence="hutchinson", step_control="trajectory").n_probes == 1
        assert cls(b=b, n_step=10, return_dlogp=True, divergence="hutchinson", n_probes=np.int64(3)).n_probes == 3
        with pytest.raises(ValueError, match="divergence"):
            cls(b=b, n_step=10, return_dlogp=True, divergence="gaussian")
        with pytest.raises(ValueError, match="return_dlogp"):
            cls(b=b, n_step=10, divergence="hutchinson")
        for bad in (0, -1, 1.0, 2.5, "2", None, True):
            with pytest.raises(ValueError, match="n_probes"):
                cls(b=b, n_step=10, return_dlogp=True, divergence="hutchinson", n_probes=bad)


def test_divergence_keywords_are_keyword_only():
    import inspect
    _, classes = _integrators()
    for cls in classes:
        params = inspect.signature(cls.__init__).parameters
        for name in ("divergence", "n_probes", "probe_seed"):
            assert params[name].kind is inspect.Parameter.KEYWORD_ONLY, name
    ti = pkg()
    b = ti.thermo.ambient.cPaiNN(n_features=32, score_layers=2, temp_length=100)
    with pytest.raises(TypeError):
        classes[0](b, "dopri5", 10, 1e-4, 1e-4, 0.0, 1.0, True, False, "hutchinson")


@pytest.mark.parametrize("which", ["sample_ambient", "sample_latent"])
def test_drivers_pass_the_config_keys(which, monkeypatch, tmp_path):
    """The drivers read divergence / n_probes / probe_seed with getattr defaults, like step_control."""
    ti = pkg()
    mod = ti.thermo.ambient if which == "sample_ambient" else ti.thermo.latent
    seen = []

    class Stop(Exception):
        pass

    class Spy(mod.MoleculeIntegrator):
        def __init__(self, *a, **kw):
            seen.append(kw)
            super().__init__(*a, **kw)
            raise Stop

    monkeypatch.setattr(mod, "MoleculeIntegrator", Spy)
    b = mod.cPaiNN(n_features=32, score_layers=2, temp_length=100)
    base = dict(seed=0, batch_size=2, n_steps=3, atol=1e-5, rtol=1e-5, return_dlogp=1, method="heun",
                data_save_path=str(tmp_path), data_save_name="x")
    fn = getattr(ti.drivers, which)
    with pytest.raises(Stop):
        fn(types.SimpleNamespace(**base), b, None)
    with pytest.raises(Stop):
        fn(types.SimpleNamespace(divergence="hutchinson", n_probes=4, probe_seed=11, **base), b, None)
    assert (seen[0]["divergence"], seen[0]["n_probes"], seen[0]["probe_seed"]) == ("exact", 1, 0)
    assert (seen[1]["divergence"], seen[1]["n_probes"], seen[1]["probe_seed"]) == ("hutchinson", 4, 11)


def test_new_symbols_are_declared_in_the_header():
    ti = pkg()
    header = open(os.path.join(ROOT, "include", "ti_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in ti._lib.ABI_SYMBOLS, name
    assert "#define TI_ABI_VERSION 5" in header                          # additive: the version stays


def test_new_entries_refuse_bad_arguments_before_the_device(lib):
    ti = pkg()
    E = ti._lib.TI_E_ARG
    assert lib.ti_painn_drift_div_est(None, None, 0.5, None, 1, 1, 0, 0, None, None, 0) == E
    assert lib.ti_painn_drift_div_est_tv(None, None, None, None, 1, 1, 0, 0, None, None, 0) == E
    grid = np.linspace(0, 1, 3).astype(np.float32)
    rd = ti.engine._rollout_desc("heun", grid, 1, 0, 0.0, 0, 0, False)
    assert lib.ti_painn_rollout_dlogp_est(None, C.byref(rd), 1, 0, None, None, 1, 1.0, 1.0, 0, None, None, None) == E
    assert "painn handle" in lib.ti_last_error().decode()
