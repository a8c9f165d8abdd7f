"""The blocked eigensolver and the wide gEDMD algebra without a GPU: the numpy restatement of ti_obs_eigh_wide (tests/eigh_wide_numpy.py)
against numpy.linalg.eigh(UPLO="U") for n in {65, 66, 96, 97, 129} x the five kinds of tests/eigh_numpy.py under the bounds of
tests/test_eigh_host.py -- eigenvalues and max |A V - V diag(w)| within 32 n 2^-53 ||A||_F, max |V^H V - I| within 32 n 2^-53 --, the C
ABI (declared, exported, listed, the refusals that need no device), the launch rule, the Python argument checks, the drivers'
`kinetics.solver` key, the code objects of the new kernels (no private segment, no spills) and the recorded ISA comparison with the
parent build.  Worst of the restatement over the 25 matrices: 8.0, 1.8 and 11.7 of the units of eigh_numpy.errors (bound: 32)."""
import ctypes as C
import functools
import os
import re
import types

import numpy as np
import pytest

from conftest import ROOT, pkg
import eigh_numpy as en
import eigh_wide_numpy as ew
from test_edge_mask_host import _kernel_metadata
from test_gedmd_wide_host import code_objects          # noqa: F401  (a fixture)

FACTOR = 32.0
# mangled-name tag -> instantiations
NEW_KERNELS = {"eigw_init_kernel": 1, "eigw_pair_kernel": 1, "eigw_update_kernel": 2, "eigw_sweep_end_kernel": 1, "eigw_finish_kernel": 1,
               "eigw_gedmd_rank_kernel": 1, "eigw_gedmd_t_kernel": 1, "eigw_gedmd_r_kernel": 1, "eigw_gedmd_back_kernel": 1}


@functools.lru_cache(maxsize=None)
def restated(kind, n):
    """(A, w, v, sweeps) of the restatement, computed once for all the tests of this module"""
    A = en.make(kind, n)
    A.setflags(write=False)
    return (A, *ew.eigh(A))


# ------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("n", ew.SIZES)
def test_restatement_against_lapack(n):
    for i, kind in enumerate(en.KINDS):
        A, w, v, sweeps = restated(kind, n)
        err = np.array(en.errors(A, w, v))
        print(f"{kind}-n{n}: outer sweeps {sweeps}, eigenvalues {err[0]:.2f}, residual {err[1]:.2f}, orthogonality {err[2]:.2f}")
        assert (np.diff(w) >= 0).all() and 1 <= sweeps <= ew.MAX_SWEEPS and sweeps == ew.SWEEPS[n][i]
        assert (err <= FACTOR).all(), (kind, n, err)
        if kind == "identity":
            assert sweeps == 1 and np.array_equal(w, np.full(n, 3.0)) and np.array_equal(v, np.eye(n))


def test_restatement_reads_the_upper_triangle_only_and_hands_narrow_orders_to_the_narrow_one():
    A, w, v, sweeps = restated("random", 65)
    dirty = A.copy()
    dirty[np.tril_indices(65, -1)] = np.nan
    dirty.imag[np.diag_indices(65)] = np.nan
    w2, v2, s2 = ew.eigh(dirty)
    assert np.array_equal(w, w2) and np.array_equal(v, v2) and sweeps == s2
    B = en.make("gram", 64)
    for got, ref in zip(ew.eigh(B), en.eigh(B)):
        assert np.array_equal(got, ref)
    bad = A.copy()
    bad[3, 40] = np.inf
    with pytest.raises(FloatingPointError):
        ew.eigh(bad)


def test_block_tournament_meets_every_block_pair_once_per_outer_sweep():
    for n in (65, 97, 129, 300, 1024):
        nb = -(-n // ew.BLOCK)
        mb = nb + (nb & 1)
        met = set()
        for r in range(mb - 1):
            I, J = en.round_pairs(mb, r)
            assert len(set(I) | set(J)) == mb                        # the pairs of a round are disjoint
            met |= {(int(i), int(j)) for i, j in zip(I, J) if j < nb}
        assert met == {(i, j) for i in range(nb) for j in range(i + 1, nb)}


def test_restated_spectrum_follows_the_lapack_route():
    """The two-solve algebra on an RFF Gram matrix of p = 70 whose singular values stay well above the cutoff (s_69 / s_0 = 1.2e-3
    against tol = 1e-4, so the rank does not hang on rounding): a first solve of order 70 and a second of order r = 70.  Bound: the
    eigenvector errors of the first solve, of order p eps, enter R = L^H ML L through L = U / s twice, so the spectra may differ by
    p eps max |d| (s_0 / s_r)^2 = 1.1e-6 here; observed 6e-14."""
    rs = np.random.RandomState(4)
    x = rs.standard_normal((400, 2))
    omega = rs.standard_normal((2, 70)) / 0.25
    M = np.exp(-1j * x @ omega)
    G = M.conj().T @ M
    d, W, r = ew.spectrum(G, omega, 1.6, 4, 1e-4)
    lam, U = np.linalg.eigh(G)
    lam, U = lam[::-1], U[:, ::-1]
    s = np.sqrt(np.maximum(lam, 0.0))
    r0 = max(int((s / s[0] >= 1e-4).sum()), 4)
    L = U[:, :r0] / s[:r0]
    R = L.conj().T @ ((-0.8) * (omega.T @ omega) * G) @ L
    ref = np.linalg.eigvalsh(0.5 * (R + R.conj().T))
    assert r == r0 == 70 and W.shape == (70, 4)
    assert np.abs(d - ref[-4:]).max() <= 70 * en.EPS * np.abs(ref).max() * (s[0] / s[r0 - 1]) ** 2


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_symbols_declared_exported_and_listed():
    ti = pkg()
    hdr = open(os.path.join(ROOT, "include", "ti_hip.h")).read()
    L = ti._lib.lib()
    assert "#define TI_EIGH_WIDE_MAX_N 1024" in hdr and "#define TI_EIGH_MAX_N 64" in hdr
    assert "int ti_obs_eigh_wide(ti_handle* h, const double* a, int64_t n_mat, int32_t n, double* w, double* v, int32_t* sweeps, int mem);" in hdr
    assert re.search(r"\bint ti_obs_gedmd_spectrum_wide\(ti_handle\* h, const double\* gram, int64_t n_mat, const double\* omega, const ti_gedmd_desc\* g,", hdr)
    for name in ("ti_obs_eigh_wide", "ti_obs_eigh_wide_launch_max", "ti_obs_gedmd_spectrum_wide"):
        assert name in ti._lib.ABI_SYMBOLS and hasattr(L, name)
    assert ti._lib.EIGH_WIDE_MAX_N == 1024 and ti._lib.EIGH_MAX_N == 64
    assert L.ti_version() == 5


def test_launch_rule_is_the_librarys():
    lm = pkg()._lib.eigh_wide_launch_max
    for n in (1, 64, 65, 300, 361, 362, 363, 724, 1024):
        assert lm(n) == ew.launch_max(n) == min(512, 2 ** 31 // (32 * n * n)), n
    assert lm(65) == 512 and lm(1024) == 64 and lm(0) == 0 and lm(1025) == 0 and lm(-3) == 0


def _vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def test_eigh_wide_refusals_before_the_device():
    ti = pkg()
    L = ti._lib.lib()
    a = np.zeros((2, 70, 70, 2))
    w, v, sw = np.full((2, 70), 7.0), np.full((2, 70, 70, 2), 7.0), np.full(2, 7, np.int32)

    def call(a_=a, w_=w, n_mat=2, n=70, mem=0):
        rc = L.ti_obs_eigh_wide(None, _vp(a_), n_mat, n, _vp(w_), _vp(v), _vp(sw), mem)
        return rc, ti._lib.last_error()

    for kw, msg in ((dict(a_=None), "a is NULL"), (dict(w_=None), "w is NULL"), (dict(mem=2), "unknown mem"), (dict(mem=-1), "unknown mem"),
                    (dict(n=0), "n must be in 1..1024"), (dict(n=1025), "n must be in 1..1024"), (dict(n_mat=0), "n_mat must be"),
                    (dict(n_mat=2 ** 20 + 2), "n_mat must be"), (dict(), "NULL handle"), (dict(n=3), "NULL handle"),
                    (dict(n=65, n_mat=2 ** 20 + 1), "NULL handle")):
        rc, text = call(**kw)
        assert rc == ti._lib.TI_E_ARG and msg in text, (kw, rc, text)
    assert (w == 7.0).all() and (v == 7.0).all() and (sw == 7).all()


def test_gedmd_spectrum_wide_refusals_before_the_device():
    ti = pkg()
    L = ti._lib.lib()
    p = 70
    gram = np.zeros((2, p, p, 2))
    om = np.ones((2, p))
    ev, vec, rank = np.full((2, 2), 7.0), np.full((2, p, 2, 2), 7.0), np.full(2, 7, np.int32)

    def call(g_=gram, omega=om, desc=True, ev_=ev, n_mat=2, d=2, p=p, nev=2, reserved=0, a=1.6, tol=1e-4, mem=0):
        g = ti._lib.GedmdDesc(d, p, nev, reserved, a, tol)
        rc = L.ti_obs_gedmd_spectrum_wide(None, _vp(g_), n_mat, None if omega is None else omega.ctypes.data_as(C.POINTER(C.c_double)),
                                          C.byref(g) if desc else None, _vp(ev_), _vp(vec), _vp(rank), mem)
        return rc, ti._lib.last_error()

    bad = om.copy()
    bad[1, 1] = np.nan
    E = ti._lib.TI_E_ARG
    for kw, code, msg in ((dict(g_=None), E, "gram is NULL"), (dict(omega=None), E, "omega is NULL"), (dict(desc=False), E, "g is NULL"),
                          (dict(ev_=None), E, "ev is NULL"), (dict(mem=2), E, "unknown mem"), (dict(p=0), E, "p must be"),
                          (dict(p=1025, omega=np.ones((2, 1025))), ti._lib.TI_E_UNSUPPORTED, "p must be <= 1024"), (dict(d=0), E, "d must be"),
                          (dict(d=17, omega=np.ones((17, p))), E, "d must be"), (dict(nev=0), E, "nev must be"), (dict(nev=p + 1), E, "nev must be"),
                          (dict(reserved=1), E, "reserved"), (dict(a=np.inf), E, "a must be finite"), (dict(tol=-1e-9), E, "tol must be"),
                          (dict(tol=np.nan), E, "tol must be"), (dict(omega=bad), E, f"non-finite omega at entry {p + 1}"),
                          (dict(n_mat=0), E, "n_mat must be"), (dict(n_mat=2 ** 20 + 2), E, "n_mat must be"), (dict(), E, "NULL handle"),
                          (dict(p=3, omega=np.ones((2, 3))), E, "NULL handle")):
        rc, text = call(**kw)
        assert rc == code and msg in text, (kw, rc, text)
    assert "host" in call(p=1025, omega=np.ones((2, 1025)))[1]
    assert (ev == 7.0).all() and (vec == 7.0).all() and (rank == 7).all()


# ------------------------------------------------------------------------------------------------------------ Python
def test_python_argument_validation():
    obs = pkg().observables
    assert obs.SOLVERS == ("host", "device")
    assert callable(obs.eigh_batched_wide) and callable(obs.gedmd_spectrum_wide) and callable(obs.gedmd_generator_wide)
    om = np.ones((1, 70))
    G = np.eye(70, dtype=np.complex128)
    for kw, msg in ((dict(nev=0), "nev"), (dict(nev=71), "nev"), (dict(a=np.inf), "finite"), (dict(tol=-1.0), "tol"), (dict(gram=np.eye(3)), "gram must be"),
                    (dict(gram=np.eye(1025), omega=np.ones((1, 1025))), "1024")):
        args = dict(gram=G, omega=om, a=1.6, nev=2, tol=0.0)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            obs.gedmd_spectrum_wide(**args)
    with pytest.raises(ValueError, match="level"):
        obs.gedmd_generator_wide(np.zeros(8, np.float32), om, 2, 1.6, level=1.0)
    with pytest.raises(ValueError, match="gedmd_spectrum_wide"):                 # the narrow refusal names the wide route
        obs.gedmd_spectrum(np.eye(65, dtype=np.complex128), np.ones((1, 65)), 1.6, 2, solver="device")


# ------------------------------------------------------------------------------------------------------------ the drivers' key
def test_kinetics_solver_key():
    dr = pkg().drivers
    ok = {"columns": [0], "temperature": 300.0}
    assert dr.KINETICS_SOLVER == "host" and dr._kinetics_solver({}) == "host" and dr._kinetics_solver({"kinetics": ok}) == "host"
    assert dr._kinetics_solver({"kinetics": {**ok, "solver": "device"}}) == "device"
    plain = dr._kinetics_settings({"kinetics": ok}, 1)
    assert plain == {"columns": [0], "p": 300, "sigma": 5.0, "nev": 4, "tol": 1e-4, "n_boot": 1000, "seed": 0, "temperature": 300.0}
    for solver in ("host", "device"):
        assert dr._kinetics_settings({"kinetics": {**ok, "solver": solver}}, 1) == plain
    for bad in ("gpu", "", None, 1):
        with pytest.raises(ValueError, match="kinetics"):
            dr._kinetics_settings({"kinetics": {**ok, "solver": bad}}, 1)
        with pytest.raises(ValueError, match="kinetics"):
            dr._kinetics_solver({"kinetics": {**ok, "solver": bad}})
    # before any rollout
    cfg = types.SimpleNamespace(observables={"descriptors": [["torsion", 0, 1, 2, 3]], "kinetics": {**ok, "solver": "gpu"}}, data_save_path="/nonexistent")
    with pytest.raises(ValueError, match="kinetics"):
        dr._check_kinetics(cfg)
    for driver in (dr.sample_ambient, dr.sample_latent):
        with pytest.raises(ValueError, match="kinetics"):
            driver(cfg, None, None)


@pytest.mark.parametrize("solver", [None, "host", "device"])
def test_kinetics_solver_routes_the_same_arguments(tmp_path, monkeypatch, solver):
    ti = pkg()
    obs, dr = ti.observables, ti.drivers
    kin = {"columns": [1, 2], "p": 7, "nev": 2, "n_boot": 5, "seed": 9, "temperature": 250.0}
    if solver is not None:
        kin["solver"] = solver
    cfg = types.SimpleNamespace(observables={"descriptors": [["rmsd"], ["torsion", 0, 1, 2, 3], ["torsion", 1, 2, 3, 4]], "bins": 4, "kinetics": kin})
    seen = {}

    def fake_summary(cv, dl, bins=32, engine=None):
        return np.zeros((cv.shape[1], bins)), np.zeros((cv.shape[1], bins + 1)), 3.5

    def fake(which):
        def generator(values, omega, nev, a, **kw):
            seen.setdefault(which, []).append(dict(values=np.asarray(values), omega=omega, nev=nev, a=a, kw=kw))
            return obs.GedmdResult(np.array([-2.0, 0.0]), np.array([[-2.5, -0.1], [-1.5, 0.1]]), np.zeros((5, 2)), np.zeros((7, 2)), 4)
        return generator

    monkeypatch.setattr(obs, "end_state_summary", fake_summary)
    monkeypatch.setattr(obs, "gedmd_generator", fake("narrow"))
    monkeypatch.setattr(obs, "gedmd_generator_wide", fake("wide"))
    rs = np.random.RandomState(1)
    cvs = [rs.rand(3, 4, 3).astype(np.float32), rs.rand(3, 2, 3).astype(np.float32)]
    dr._write_observables(cfg, str(tmp_path / "out.npz"), cvs, [])
    z = np.load(tmp_path / "out.npz")
    assert sorted(z.files) == ["cv", "edges", "ess", "hist", "kinetics_ci", "kinetics_eigenvalues", "kinetics_rank"]
    np.testing.assert_array_equal(z["kinetics_eigenvalues"], [-2.0, 0.0])
    assert int(z["kinetics_rank"]) == 4
    assert sorted(seen) == (["wide"] if solver == "device" else ["narrow"])
    (call,) = seen["wide" if solver == "device" else "narrow"]
    np.testing.assert_array_equal(call["values"], np.concatenate(cvs, axis=1)[-1][:, 1:3])
    assert call["values"].dtype == np.float32 and call["nev"] == 2 and call["a"] == dr.KINETICS_KB * 250.0
    np.testing.assert_array_equal(call["omega"], obs.sample_rff_gaussian(2, 7, 5.0, 9))
    assert call["kw"] == dict(tol=1e-4, n_boot=5, seed=9)


# ------------------------------------------------------------------------------------------------------------ code objects
def test_new_kernels_exist_without_scratch_or_spills(code_objects):
    meta = {}
    for co in code_objects:
        meta.update(_kernel_metadata(co))
    for tag, count in NEW_KERNELS.items():
        hits = {n: m for n, m in meta.items() if f"{len(tag)}{tag}" in n}
        assert len(hits) == count, (tag, sorted(hits))
        assert set(hits.values()) == {(0, 0, 0)}, hits


def test_recorded_isa_comparison_with_the_parent_build():
    """tools/isa_compare.py PARENT.so THIS.so, recorded: every kernel of the parent is instruction-identical (obs_eigh_kernel and the
    narrow gEDMD kernels included: the blocked solver keeps a copy of the Jacobi sweep), the ten kernels above are added."""
    text = open(os.path.join(ROOT, "profiles", "eigh_wide_isa_compare.txt")).read()
    m = re.search(r"(\d+) symbols in \S+; identical in \S+: (\d+); differing: (\d+); missing: (\d+); added: (\d+)", text)
    assert m, text[:400]
    total, same, diff, missing, added = map(int, m.groups())
    assert total == same and diff == 0 and missing == 0
    added_names = re.findall(r"^ADDED (.*)$", text, flags=re.M)
    assert added == len(added_names) == sum(NEW_KERNELS.values())
    for tag in NEW_KERNELS:
        assert any(tag in n for n in added_names), tag
