"""Boltzmann-generator weights on the host: the C ABI's declaration, listing and export, the refusals that need no device, the numpy
restatement (tests/bg_numpy.py) against the reference's own functions (tests/golden/bg_reference.npz, make_golden_bg.py), and the
drivers' new key observables["bg"], checked before any rollout.  No GPU.

Bounds against the fixture, with m = 3A terms in the sum of squares:
    |logpz - ref| <= m 2^-50 |ref|                                        the forward error of an m-term fp64 sum, slack 8
    |logw - log w_ref| <= 2^-24 |log w_ref| + m 2^-50 (|E1| + |logpz| + |nb| + |nt|)   one fp32 rounding plus the fp64 terms
Worst ratios of the restatement to the two bars on the fixture's inputs: 0.008 and 0.960."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT, pkg
import bg_numpy as bgn

GOLDEN = os.path.join(ROOT, "tests", "golden", "bg_reference.npz")
XML = os.path.join(ROOT, "tests", "golden", "ff_small.xml")


def fixture_cases():
    """the fixture's cases as dicts: name, A, m, z [50, m], E1, nd_bg, nd_ti, log_pz, w, ess, ess_k, kept_k, ess_k_ok, k"""
    f = np.load(GOLDEN)
    out = []
    for c, name in enumerate(f["names"]):
        A, rows = int(f["A"][c]), slice(int(f["off"][c]), int(f["off"][c + 1]))
        z = f["z_flat"][int(f["zoff"][c]):int(f["zoff"][c + 1])].reshape(-1, 3 * A)
        out.append(dict(name=str(name), A=A, m=3 * A, z=z, E1=f["E1"][rows], nd_bg=f["nd_bg"][rows], nd_ti=f["nd_ti"][rows],
                        log_pz=f["log_pz"][rows], w=f["w"][rows], ess=float(f["ess"][c]), ess_k=float(f["ess_k"][c]),
                        kept_k=int(f["kept_k"][c]), ess_k_ok=bool(f["ess_k_ok"][c]), k=float(f["k"])))
    return out


def check_against_fixture(c, logpz, logw, worst):
    """the two bounds of the module docstring; worst[0], worst[1] collect the largest fractions of them"""
    m, ref_lw = c["m"], np.log(c["w"])
    bar_pz = m * 2.0 ** -50 * np.abs(c["log_pz"])
    bar_lw = 2.0 ** -24 * np.abs(ref_lw) + m * 2.0 ** -50 * (np.abs(c["E1"]) + np.abs(c["log_pz"]) + np.abs(c["nd_bg"]) + np.abs(c["nd_ti"]))
    e_pz, e_lw = np.abs(np.asarray(logpz, np.float64) - c["log_pz"]), np.abs(np.asarray(logw).astype(np.float64) - ref_lw)
    worst[0], worst[1] = max(worst[0], (e_pz / bar_pz).max()), max(worst[1], (e_lw / bar_lw).max())
    assert (e_pz <= bar_pz).all(), (c["name"], (e_pz / bar_pz).max())
    assert (e_lw <= bar_lw).all(), (c["name"], (e_lw / bar_lw).max())


# ---- 1. the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbol_declared_listed_and_exported():
    ti = pkg()
    hdr = open(os.path.join(ROOT, "include", "ti_hip.h")).read()
    L = ti._lib.lib()
    assert re.search(r"\bint ti_obs_bg_logw\(ti_handle\* h, const float\* z, int64_t B, int64_t m, const double\* u1, "
                     r"const float\* neg_dlogp_bg, const float\* neg_dlogp_ti,\s+double\* out_logpz, float\* out_logw, int mem\);", hdr)
    assert "ti_obs_bg_logw" in ti._lib.ABI_SYMBOLS and hasattr(L, "ti_obs_bg_logw")
    assert re.search(r"\bint ti_obs_bg_ess\(ti_handle\* h, const double\* logpz, int64_t B, const double\* u1, ", hdr)
    assert "ti_obs_bg_ess" in ti._lib.ABI_SYMBOLS and hasattr(L, "ti_obs_bg_ess")
    assert "obs_bg_kernels.hip" in ti.build.SOURCES
    assert L.ti_version() == 5 and "#define TI_ABI_VERSION 5" in hdr                 # additive: the version stays
    assert "#define TI_BG_MAX_M 65536" in hdr and "#define TI_BG_HALF_LOG_2PI 0.9189385332046727" in hdr
    assert (ti._lib.BG_MAX_M, ti._lib.BG_HALF_LOG_2PI) == (65536, bgn.HALF_LOG_2PI)
    assert bgn.HALF_LOG_2PI == 0.5 * np.log(2.0 * np.pi)


def test_refusals_before_the_device():
    """every refusal of the entry point needs no device and is made before the handle is looked at; nothing is written"""
    ti = pkg()
    L, E = ti._lib.lib(), ti._lib.TI_E_ARG
    z = np.ones((2, 3), np.float32)
    lp, lw = np.full(2, 7.0), np.full(2, 7.0, np.float32)
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
    call = lambda z_, B, m, lp_, lw_, mem: L.ti_obs_bg_logw(None, p(z_), B, m, None, None, None, p(lp_), p(lw_), mem)
    for args, msg in (((None, 2, 3, lp, lw, 0), "z is NULL"), ((z, 2, 3, None, None, 0), "both NULL"), ((z, 2, 3, lp, lw, 2), "unknown mem"),
                      ((z, 0, 3, lp, lw, 0), "B < 1"), ((z, -1, 3, lp, lw, 0), "B < 1"), ((z, 2, 0, lp, lw, 0), "m must be in 1..65536"),
                      ((z, 2, 65537, lp, lw, 0), "m must be in 1..65536"), ((z, 2, 3, lp, lw, 0), "NULL handle"),
                      ((z, 2, 3, None, lw, 1), "NULL handle"), ((z, 2, 3, lp, None, 0), "NULL handle")):
        assert call(*args) == E, msg
        assert msg in ti._lib.last_error(), (msg, ti._lib.last_error())
    assert (lp == 7.0).all() and (lw == 7.0).all()
    ess = C.c_double(7.0)
    for args, msg in (((None, 2, C.byref(ess), 0), "NULL buffer"), ((p(lp), 2, None, 0), "NULL buffer"), ((p(lp), 2, C.byref(ess), 2), "unknown mem"),
                      ((p(lp), 0, C.byref(ess), 0), "B < 1"), ((p(lp), 2, C.byref(ess), 0), "NULL handle")):
        assert L.ti_obs_bg_ess(None, args[0], args[1], None, None, None, None, args[2], None, args[3]) == E, msg
        assert msg in ti._lib.last_error(), (msg, ti._lib.last_error())
    assert ess.value == 7.0


def test_engine_layer_refusals_need_no_handle():
    ti = pkg()
    eng = object.__new__(ti.engine.AdwEngine)
    with pytest.raises(ValueError, match="non-empty"):
        eng.bg_logw(np.zeros((0, 3), np.float32))
    with pytest.raises(ValueError, match="1..65536"):
        eng.bg_logw(np.zeros((2, 0), np.float32))
    with pytest.raises(ValueError, match="1..65536"):
        eng.bg_logw(np.zeros((1, 65537), np.float32))
    with pytest.raises(ValueError, match="neg_dlogp_bg must have shape"):
        eng.bg_logw(np.zeros((2, 3), np.float32), None, np.zeros(3, np.float32))
    for cls in (ti.engine.PainnEngine, ti.engine.AdwEngine):
        assert cls.bg_logw is ti.engine._Engine.bg_logw and cls.ti_logw is ti.engine._Engine.ti_logw     # on the class that owns ti_logw
    for name in ("log_prior", "bg_logw", "ess_bg", "free_energy_bg_tfep"):
        assert callable(getattr(ti.observables, name))
    assert "build-defined" in ti.thermo.latent.MoleculeIntegrator.log_prob.__doc__.lower()


# ---- 2. the restatement ------------------------------------------------------------------------------------------------------------
def test_restatement_by_hand():
    """lane order and butterfly on cases small enough to write out; the absent terms; the product rounded before the subtraction"""
    z = np.array([[1.0, 2.0, 3.0]], np.float32)
    lp, lw = bgn.bg_logw(z)
    assert lp[0] == -(0.5 * 14.0) - (3.0 * bgn.HALF_LOG_2PI) and lw[0] == np.float32(-lp[0])
    # m = 65: lane 0 holds z[0]^2 + z[64]^2, the butterfly pairs lane l with l ^ 32 first
    z = (np.arange(65, dtype=np.float32) * np.float32(1.0009765625) + np.float32(1e-3)).reshape(1, 65)
    v = z[0].astype(np.float64) ** 2
    lanes = np.zeros(64)
    lanes[:] = v[:64]
    lanes[0] = v[0] + v[64]
    s = lanes.copy()
    for o in (32, 16, 8, 4, 2, 1):
        s = np.array([s[l] + s[l ^ o] for l in range(64)])
    assert len(set(s.tolist())) == 1
    assert bgn.log_prior(z)[0] == -(0.5 * s[0]) - (65.0 * bgn.HALF_LOG_2PI)
    u1, nb, nt = np.array([3.25]), np.array([0.1], np.float32), np.array([-7.3], np.float32)
    lp, lw = bgn.bg_logw(z, u1, nb, nt)
    assert lw[0] == np.float32(-(((3.25 + lp[0]) + float(nb[0])) + float(nt[0])))
    # exact terms: the square of an fp32 value has at most 48 significant bits
    x = np.float32(1.0) + np.float32(2.0 ** -23)
    assert float(x) * float(x) == 1.0 + 2.0 ** -22 + 2.0 ** -46
    # non-finite rows stay in their rows
    z = np.ones((3, 5), np.float32)
    z[1, 2] = np.inf
    lp = bgn.log_prior(z)
    assert lp[1] == -np.inf and lp[0] == lp[2] == -(0.5 * 5.0) - (5.0 * bgn.HALF_LOG_2PI)


def test_restatement_against_the_reference_fixture():
    worst = [0.0, 0.0]
    cases = fixture_cases()
    assert [c["A"] for c in cases] == [1, 9, 18, 21, 22, 32, 18] and all(c["z"].shape == (50, c["m"]) for c in cases)
    assert (cases[-1]["nd_ti"] == 0).all() and all((c["nd_ti"] != 0).any() for c in cases[:-1])
    assert all(np.isfinite(c["w"]).all() and (c["w"] > 0).all() for c in cases) and any(c["ess_k_ok"] for c in cases)
    for c in cases:
        lp, lw = bgn.bg_logw(c["z"], c["E1"], c["nd_bg"], c["nd_ti"])
        check_against_fixture(c, lp, lw, worst)
    print(f"restatement against the reference: worst errors {worst[0]:.3f} and {worst[1]:.3f} of the bounds")
    assert os.path.getsize(GOLDEN) < 128 * 1024


# ---- 3. the driver key -------------------------------------------------------------------------------------------------------------
class _Untouchable:
    """A model or dataset stand-in: any use of it means the driver went past its checks"""
    def __getattr__(self, name):
        raise AssertionError(f"the driver touched its argument ({name}) before refusing the key")


def _cfg(tmp_path, obs, **kw):
    return types.SimpleNamespace(observables=obs, data_save_path=str(tmp_path / "out"), data_save_name="bg", **{"return_dlogp": 1, **kw})


def test_sample_latent_checks_the_key_before_any_rollout(tmp_path):
    ti = pkg()
    dr = ti.drivers
    good = {"forcefield": XML, "scale": 2.0}
    for bad, msg in (({"forcefield": XML}, "exactly the keys"), ({**good, "extra": 1}, "exactly the keys"), (True, "exactly the keys"), ("x", "exactly the keys"),
                     ({**good, "scale": 0.0}, "scale"), ({**good, "scale": True}, "scale"), ({**good, "scale": float("nan")}, "scale")):
        with pytest.raises(ValueError, match=r"observables\['bg'\].*" + msg):
            dr.sample_latent(_cfg(tmp_path, {"bg": bad}), _Untouchable(), _Untouchable())
    with pytest.raises(ValueError, match=r"observables\['bg'\] needs return_dlogp"):
        dr.sample_latent(_cfg(tmp_path, {"bg": good}, return_dlogp=0), _Untouchable(), _Untouchable())
    with pytest.raises((OSError, ValueError)):                                            # the force field is read before the rollout
        dr.sample_latent(_cfg(tmp_path, {"bg": {"forcefield": str(tmp_path / "missing.xml"), "scale": 2.0}}), _Untouchable(), _Untouchable())
    # the energy key keeps its refusal
    with pytest.raises(ValueError, match="log p"):
        dr.sample_latent(_cfg(tmp_path, {"energy": good}), _Untouchable(), _Untouchable())
    assert not os.path.exists(tmp_path / "out")
    ff, to_nm = dr._check_bg(_cfg(tmp_path, {"bg": good}), "sample_latent")
    assert to_nm == 0.5 and ff is not None
    assert dr._check_bg(_cfg(tmp_path, {"descriptors": [["dist", 0, 1]]}), "sample_latent") is None
    assert dr._check_bg(types.SimpleNamespace(), "sample_latent") is None


def test_sample_ambient_checks_the_key_before_any_rollout(tmp_path):
    ti = pkg()
    dr = ti.drivers
    energy, desc = {"forcefield": XML, "scale": 2.0}, [["dist", 0, 1]]
    with pytest.raises(ValueError, match=r"observables\['bg'\] must be true"):
        dr.sample_ambient(_cfg(tmp_path, {"descriptors": desc, "energy": energy, "bg": energy}), _Untouchable(), _Untouchable())
    with pytest.raises(ValueError, match=r"observables\['bg'\] needs observables\['energy'\]"):
        dr.sample_ambient(_cfg(tmp_path, {"descriptors": desc, "bg": True}), _Untouchable(), _Untouchable())
    with pytest.raises(ValueError, match=r"observables\['bg'\].*descriptors"):
        dr.sample_ambient(_cfg(tmp_path, {"energy": energy, "bg": True}), _Untouchable(), _Untouchable())
    for dataset in (types.SimpleNamespace(), types.SimpleNamespace(use_latent_trajs=False)):
        with pytest.raises(ValueError, match="use_latent_trajs"):
            dr.sample_ambient(_cfg(tmp_path, {"descriptors": desc, "energy": energy, "bg": True}), _Untouchable(), dataset)
    assert not os.path.exists(tmp_path / "out")
    ok = _cfg(tmp_path, {"descriptors": desc, "energy": energy, "bg": True})
    assert dr._check_bg(ok, "sample_ambient", types.SimpleNamespace(use_latent_trajs=True)) is True
    assert dr._check_bg(_cfg(tmp_path, {"descriptors": desc, "bg": False}), "sample_ambient", _Untouchable()) is None
    # the dataset says how it was built
    src = open(os.path.join(ROOT, "thermodynamic-interpolation_amd", "data.py")).read()
    assert "self.use_latent_trajs = bool(use_latent_trajs)" in src


def test_sample_adw_refuses_the_key():
    ti = pkg()
    cfg = types.SimpleNamespace(observables={"descriptors": [["coord", 0]], "bg": True}, beta0s=[1.0], beta1s=[1.25], return_dlogp=1)
    with pytest.raises(ValueError, match=r"observables\['bg'\] is for sample_latent / sample_ambient"):
        ti.drivers.sample_adw(cfg, types.SimpleNamespace(dim=1), _Untouchable())


def test_observe_kw_drops_the_key():
    ti = pkg()
    dr = ti.drivers
    bg = {"forcefield": XML, "scale": 2.0}
    cfg = types.SimpleNamespace(observables={"descriptors": [["dist", 0, 1]], "bg": bg, "bootstrap": 8})
    assert dr._observe_kw(cfg)["observe"] == {"descriptors": [["dist", 0, 1]]}
    assert dr._observe_kw(types.SimpleNamespace(observables={"bg": bg, "bootstrap": 8})) == {}      # weights without CVs: no observer
    assert dr._observe_kw(types.SimpleNamespace(observables={"descriptors": [["dist", 0, 1]], "bg": True, "energy": bg}))["observe"] == \
        {"descriptors": [["dist", 0, 1]]}
    assert "observe" in dr._observe_kw(types.SimpleNamespace(observables={"bootstrap": 8}))          # without the key: as before
