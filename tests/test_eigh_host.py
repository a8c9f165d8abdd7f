"""The batched Hermitian eigensolver and the device gEDMD algebra without a GPU: the numpy restatement of the Jacobi scheme
(tests/eigh_numpy.py, written from include/ti_hip.h) against LAPACK on the 45 matrices the GPU test uses, the restatement through the
spectrum algebra against the reference fixture, the C ABI of ti_obs_eigh and ti_obs_gedmd_spectrum (declared, exported, listed, the
refusals that need no device), the Python argument checks, and the code objects of the new kernels (no private segment, no spills).

Bounds: eigenvalues and max |A V - V diag(w)| within 32 n 2^-53 ||A||_F, max |V^H V - I| within 32 n 2^-53 -- n eps ||A||_F is the
backward-error form of Jacobi.  Worst observed for the restatement over the 45 matrices: 3.7, 1.4 and 7.0 of those units."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, pkg
import eigh_numpy as en
import gedmd_numpy as gn
from test_edge_mask_host import _kernel_metadata
from test_gedmd_host import code_objects, fixture_cases          # noqa: F401  (code_objects is a fixture)

NEW_KERNELS = ("obs_eigh_kernel", "obs_gedmd_reduce_kernel", "obs_gedmd_back_kernel")
FACTOR = 32.0


# ------------------------------------------------------------------------------------------------------------ the oracle
def test_the_45_matrices_are_what_the_issue_lists():
    cs = en.cases()
    assert len(cs) == 45 and en.SIZES == (1, 2, 3, 15, 16, 17, 33, 63, 64) and len(en.KINDS) == 5
    for name, A in cs:
        assert np.array_equal(A, A.conj().T) and (A.imag.diagonal() == 0).all(), name
    g = dict(cs)
    lam = np.linalg.eigvalsh(g["gram-n64"])
    assert abs(lam[-1] / 4096.0 - 1) < 1e-12 and lam[0] < 1e-12 * lam[-1]                  # numerically rank-deficient
    np.testing.assert_allclose(np.unique(np.round(np.linalg.eigvalsh(g["degenerate-n64"]), 9)), [-1.0, 2.0, 5.0])
    assert np.linalg.matrix_rank(g["rank1-n33"]) == 1
    assert np.array_equal(g["identity-n17"], 3 * np.eye(17))


@pytest.mark.parametrize("n", en.SIZES)
def test_restatement_against_lapack(n):
    worst = np.zeros(3)
    for kind in en.KINDS:
        A = en.make(kind, n)
        w, v, sweeps = en.eigh(A)
        err = np.array(en.errors(A, w, v))
        print(f"{kind}-n{n}: sweeps {sweeps}, eigenvalues {err[0]:.2f}, residual {err[1]:.2f} (n eps ||A||_F), orthogonality {err[2]:.2f} (n eps)")
        worst = np.maximum(worst, err)
        assert (np.diff(w) >= 0).all() and 1 <= sweeps <= en.MAX_SWEEPS
        assert (err <= FACTOR).all(), (kind, n, err)
        if kind == "identity":
            assert sweeps == 1 and np.array_equal(w, np.full(n, 3.0)) and np.array_equal(v, np.eye(n))
    print(f"n = {n}: worst {worst}")


def test_restatement_reads_the_upper_triangle_only_and_orders_ties_by_position():
    A = en.make("random", 17)
    dirty = A.copy()
    dirty[np.tril_indices(17, -1)] = np.nan
    dirty[np.diag_indices(17)] += 1j * 5.0
    for a, b in zip(en.eigh(A), en.eigh(dirty)):
        assert np.array_equal(a, b)
    w, v, sweeps = en.eigh(np.diag([2.0, 1.0, 2.0, 1.0]))
    assert sweeps == 1 and np.array_equal(w, [1, 1, 2, 2]) and np.array_equal(v, np.eye(4)[:, [1, 3, 0, 2]])
    with pytest.raises(FloatingPointError):
        en.eigh(np.array([[1.0, np.inf], [0.0, 1.0]]))


def test_tournament_meets_every_pair_once_per_sweep():
    for m in (2, 4, 16, 34, 64):
        seen = set()
        for r in range(m - 1):
            p, q = en.round_pairs(m, r)
            assert (p < q).all() and len(set(p) | set(q)) == m                              # disjoint pairs
            seen |= set(zip(p.tolist(), q.tolist()))
        assert len(seen) == m * (m - 1) // 2


def test_restatement_through_the_spectrum_algebra_reproduces_the_fixture():
    """All 28 fixture rows: equal ranks, eigenvalues within 64 ev_dev (the project's allowance for the LAPACK route)."""
    cases, ev_dev = fixture_cases()
    worst, rows = 0.0, 0
    for c in cases:
        for i, row in enumerate([None, *c["idx"]]):
            G = gn.gram(c["x"], c["omega"], row)
            d, W, r = en.spectrum(G, c["omega"], c["a"], c["nev"], c["tol"])
            assert r == c["rank"][i], (c["name"], i)
            worst, rows = max(worst, np.abs(d - c["ev"][i]).max()), rows + 1
            assert np.abs(d - c["ev"][i]).max() <= 64 * ev_dev, (c["name"], i)
            np.testing.assert_allclose(W.conj().T @ G @ W, np.eye(c["nev"]), atol=1e-7)
    assert rows == 28
    print(f"Jacobi restatement against the reference: worst {worst:.2e} = {worst / ev_dev:.2f} ev_dev")


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_symbols_declared_exported_and_listed():
    ti = pkg()
    hdr = open(os.path.join(ROOT, "include", "ti_hip.h")).read()
    L = ti._lib.lib()
    assert "#define TI_EIGH_MAX_N 64" in hdr
    assert "int ti_obs_eigh(ti_handle* h, const double* a, int64_t n_mat, int32_t n, double* w, double* v, int32_t* sweeps, int mem);" in hdr
    assert "typedef struct { int32_t d, p, nev, reserved; double a, tol; } ti_gedmd_desc;" in hdr
    assert re.search(r"\bint ti_obs_gedmd_spectrum\(ti_handle\* h, const double\* gram, int64_t n_mat, const double\* omega, const ti_gedmd_desc\* g,", hdr)
    for name in ("ti_obs_eigh", "ti_obs_gedmd_spectrum"):
        assert name in ti._lib.ABI_SYMBOLS and hasattr(L, name)
    assert C.sizeof(ti._lib.GedmdDesc) == 32
    assert ti._lib.EIGH_MAX_N == 64 and ti._lib.EIGH_MAX_MATRICES == ti._lib.BOOT_MAX_RESAMPLES + 1
    assert L.ti_version() == 5


def _vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def test_eigh_refusals_before_the_device():
    ti = pkg()
    L = ti._lib.lib()
    a = np.zeros((2, 3, 3, 2))
    w, v, sw = np.full((2, 3), 7.0), np.full((2, 3, 3, 2), 7.0), np.full(2, 7, np.int32)

    def call(a_=a, w_=w, n_mat=2, n=3, mem=0):
        rc = L.ti_obs_eigh(None, _vp(a_), n_mat, n, _vp(w_), _vp(v), _vp(sw), mem)
        return rc, ti._lib.last_error()

    for kw, msg in ((dict(a_=None), "a is NULL"), (dict(w_=None), "w is NULL"), (dict(mem=2), "unknown mem"), (dict(mem=-1), "unknown mem"),
                    (dict(n=0), "n must be"), (dict(n=65), "n must be"), (dict(n_mat=0), "n_mat must be"), (dict(n_mat=2 ** 20 + 2), "n_mat must be"),
                    (dict(), "NULL handle"), (dict(n=64, n_mat=2 ** 20 + 1), "NULL handle")):
        rc, text = call(**kw)
        assert rc == ti._lib.TI_E_ARG and msg in text, (kw, rc, text)
    assert (w == 7.0).all() and (v == 7.0).all() and (sw == 7).all()


def test_gedmd_spectrum_refusals_before_the_device():
    ti = pkg()
    L = ti._lib.lib()
    gram = np.zeros((2, 3, 3, 2))
    om = np.ones((2, 3))
    ev, vec, rank = np.full((2, 2), 7.0), np.full((2, 3, 2, 2), 7.0), np.full(2, 7, np.int32)

    def call(g_=gram, omega=om, desc=True, ev_=ev, n_mat=2, d=2, p=3, nev=2, reserved=0, a=1.6, tol=1e-4, mem=0):
        g = ti._lib.GedmdDesc(d, p, nev, reserved, a, tol)
        rc = L.ti_obs_gedmd_spectrum(None, _vp(g_), n_mat, None if omega is None else omega.ctypes.data_as(C.POINTER(C.c_double)),
                                     C.byref(g) if desc else None, _vp(ev_), _vp(vec), _vp(rank), mem)
        return rc, ti._lib.last_error()

    bad = om.copy()
    bad[1, 1] = np.nan
    E = ti._lib.TI_E_ARG
    for kw, code, msg in ((dict(g_=None), E, "gram is NULL"), (dict(omega=None), E, "omega is NULL"), (dict(desc=False), E, "g is NULL"),
                          (dict(ev_=None), E, "ev is NULL"), (dict(mem=2), E, "unknown mem"), (dict(p=0), E, "p must be"),
                          (dict(p=65, omega=np.ones((2, 65))), ti._lib.TI_E_UNSUPPORTED, "p must be <= 64"), (dict(d=0), E, "d must be"),
                          (dict(d=17, omega=np.ones((17, 3))), E, "d must be"), (dict(nev=0), E, "nev must be"), (dict(nev=4), E, "nev must be"),
                          (dict(reserved=1), E, "reserved"), (dict(a=np.inf), E, "a must be finite"), (dict(a=np.nan), E, "a must be finite"),
                          (dict(tol=-1e-9), E, "tol must be"), (dict(tol=np.nan), E, "tol must be"), (dict(tol=np.inf), E, "tol must be"),
                          (dict(omega=bad), E, "non-finite omega at entry 4"), (dict(n_mat=0), E, "n_mat must be"), (dict(n_mat=2 ** 20 + 2), E, "n_mat must be"),
                          (dict(), E, "NULL handle")):
        rc, text = call(**kw)
        assert rc == code and msg in text, (kw, rc, text)
    assert "host" in call(p=65, omega=np.ones((2, 65)))[1]                     # the refusal points to the host route
    assert (ev == 7.0).all() and (vec == 7.0).all() and (rank == 7).all()


def test_python_argument_validation():
    ti = pkg()
    obs = ti.observables
    om = np.ones((1, 4))
    G = np.eye(4, dtype=np.complex128)
    with pytest.raises(ValueError, match="solver"):
        obs.gedmd_spectrum(G, om, 1.6, 2, solver="gpu")
    with pytest.raises(ValueError, match="solver"):
        obs.gedmd_generator(np.zeros(8, np.float32), om, 2, 1.6, solver="lapack")
    with pytest.raises(ValueError, match="64"):
        obs.gedmd_spectrum(np.eye(65, dtype=np.complex128), np.ones((1, 65)), 1.6, 2, solver="device")
    with pytest.raises(ValueError, match="64"):
        obs.gedmd_generator(np.zeros(8, np.float32), np.ones((1, 65)), 2, 1.6, solver="device")
    for kw, msg in ((dict(nev=0), "nev"), (dict(nev=5), "nev"), (dict(a=np.inf), "finite"), (dict(tol=-1.0), "tol"), (dict(gram=np.eye(3)), "gram must be")):
        args = dict(gram=G, omega=om, a=1.6, nev=2, tol=0.0, solver="device")
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            obs.gedmd_spectrum(**args)
    assert obs.SOLVERS == ("host", "device") and callable(obs.eigh_batched)
    # the default is the host route, bit for bit what it was: no engine is needed
    d, W, r = obs.gedmd_spectrum(2.0 * G, om, 1.6, 2)
    d2, W2, r2 = obs.gedmd_spectrum(2.0 * G, om, 1.6, 2, solver="host")
    assert np.array_equal(d, d2) and np.array_equal(W, W2) and np.array_equal(r, r2)


def test_driver_key():
    dr = pkg().drivers
    assert dr.GEDMD_SOLVER == "host" and dr._gedmd_solver({"gedmd": {"p": 8}}) == "host" and dr._gedmd_solver({}) == "host"
    assert dr._gedmd_solver({"gedmd": {"p": 8, "solver": "device"}}) == "device"
    assert dr._gedmd_settings({"gedmd": {"p": 8, "solver": "device"}})["p"] == 8
    for bad in ({"solver": "gpu"}, {"solver": "device", "p": 65, "nev": 4}):
        with pytest.raises(ValueError, match="gedmd"):
            dr._gedmd_settings({"gedmd": bad})


# ------------------------------------------------------------------------------------------------------------ code objects
def test_new_kernels_exist_without_scratch_or_spills(code_objects):
    meta = {}
    for co in code_objects:
        meta.update(_kernel_metadata(co))
    for tag in NEW_KERNELS:
        hits = {n: m for n, m in meta.items() if f"{len(tag)}{tag}" in n}
        assert len(hits) == 1, (tag, sorted(hits))
        assert set(hits.values()) == {(0, 0, 0)}, hits
    assert not [n for n in meta if "obs_gram_kernel" in n and any(t in n for t in NEW_KERNELS)]


def test_recorded_isa_comparison_with_the_parent_build():
    """tools/isa_compare.py PARENT.so THIS.so, recorded: every kernel of the parent is instruction-identical, the three above are added."""
    text = open(os.path.join(ROOT, "profiles", "eigh_isa_compare.txt")).read()
    m = re.search(r"(\d+) symbols in \S+; identical in \S+: (\d+); differing: (\d+); missing: (\d+); added: (\d+)", text)
    assert m, text[:400]
    total, same, diff, missing, added = map(int, m.groups())
    assert total == same and diff == 0 and missing == 0
    added_names = re.findall(r"^ADDED (.*)$", text, flags=re.M)
    assert added == len(added_names) == len(NEW_KERNELS)
    for tag in NEW_KERNELS:
        assert any(tag in n for n in added_names), tag
