"""Generator EDMD on random Fourier features without a GPU: the numpy restatement (tests/gedmd_numpy.py: eigh of the Gram matrix)
against the reference's SVD route (tests/golden/gedmd_reference.npz, written by tests/golden/make_golden_gedmd.py), the host algebra of
observables.gedmd_spectrum against the restatement, the C ABI of ti_obs_rff_gram (declared, exported, listed, the refusals that need
no device), the argument checks of observables.py, and the code objects of the new kernels (no private segment, no spills)."""
import ctypes as C
import os
import re
import tempfile

import numpy as np
import pytest

from conftest import ROOT, load_golden, pkg
import gedmd_numpy as gn
import test_build_isa as isa_rules
from test_edge_mask_host import _kernel_metadata

NEW_KERNELS = {"obs_gram_feature_kernel": 1, "obs_gram_reduce_kernel": 1, "obs_gram_kernel": 8}      # tag: instantiations


def fixture_cases():
    """The recorded cases as dicts: x [m, d] fp32, omega [d, p], idx [3, m] int32, ev [4, nev] (row 0: the whole sample), rank [4]"""
    g = load_golden("gedmd_reference")
    cases = []
    for c, (d, p, m, nev) in enumerate(g["cases"]):
        cases.append(dict(
            name=f"d{d}-p{p}-m{m}", d=int(d), p=int(p), m=int(m), nev=int(nev), a=float(g["a"]), tol=float(g["tol"]),
            x=g["x_flat"][g["x_off"][c]:g["x_off"][c + 1]].reshape(m, d), omega=g["omega_flat"][g["om_off"][c]:g["om_off"][c + 1]].reshape(d, p),
            idx=g["idx_flat"][g["idx_off"][c]:g["idx_off"][c + 1]].astype(np.int32).reshape(3, m), ev=g["ev"][c][:, :nev], rank=g["rank"][c]))
    return cases, float(g["ev_dev"])


# ------------------------------------------------------------------------------------------------------------ the oracle
def test_restatement_reproduces_the_reference_fixture():
    """Ranks equal, eigenvalues within 64 ev_dev: both sides are fp64 LAPACK; ev_dev is their difference where the fixture was
    written, the factor allows for another BLAS / LAPACK build."""
    cases, ev_dev = fixture_cases()
    assert [(c["d"], c["p"], c["m"], c["nev"]) for c in cases] == [(1, 50, 4097, 4), (1, 50, 1000, 4), (1, 16, 257, 4), (2, 24, 1000, 4), (3, 17, 600, 3),
                                                                  (16, 32, 2000, 4), (1, 8, 65, 2)]
    assert 0 < ev_dev < 1e-9 and all(c["x"].dtype == np.float32 for c in cases)
    assert any(c["rank"].min() < c["p"] for c in cases)                 # the cutoff binds somewhere
    worst = 0.0
    for c in cases:
        for i, row in enumerate([None, *c["idx"]]):
            d, W, r = gn.spectrum(gn.gram(c["x"], c["omega"], row), c["omega"], c["a"], c["nev"], c["tol"])
            assert r == c["rank"][i], (c["name"], i)
            assert W.shape == (c["p"], c["nev"])
            worst = max(worst, np.abs(d - c["ev"][i]).max())
            assert np.abs(d - c["ev"][i]).max() <= 64 * ev_dev, (c["name"], i)
            d2, r2 = gn.svd_route(c["x"][row] if row is not None else c["x"], c["omega"], c["a"], c["nev"], c["tol"])
            assert r2 == r and np.abs(d2 - c["ev"][i]).max() <= 64 * ev_dev
    print(f"restatement against the reference: worst {worst:.2e} (ev_dev {ev_dev:.2e})")


def test_product_spectrum_is_the_restated_one_batched():
    """observables.gedmd_spectrum over a stack of Gram matrices of differing rank = the restatement matrix by matrix."""
    obs = pkg().observables
    cases, ev_dev = fixture_cases()
    for c in cases:
        G = np.stack([gn.gram(c["x"], c["omega"], row) for row in [None, *c["idx"]]])
        d, W, r = obs.gedmd_spectrum(G, c["omega"], c["a"], c["nev"], c["tol"])
        assert d.shape == (4, c["nev"]) and W.shape == (4, c["p"], c["nev"]) and r.shape == (4,)
        np.testing.assert_array_equal(r, c["rank"])
        assert np.abs(d - c["ev"]).max() <= 64 * ev_dev, c["name"]
        # the eigenvectors: W^H G W = 1 and W^H ML W = diag(d) (any phase)
        ML = -0.5 * c["a"] * (c["omega"].T @ c["omega"]) * G[0]
        np.testing.assert_allclose(W[0].conj().T @ G[0] @ W[0], np.eye(c["nev"]), atol=1e-7)
        np.testing.assert_allclose(W[0].conj().T @ ML @ W[0], np.diag(d[0]), atol=1e-6)
        d1, W1, r1 = obs.gedmd_spectrum(G[2], c["omega"], c["a"], c["nev"], c["tol"])             # no leading axis
        assert d1.shape == (c["nev"],) and W1.shape == (c["p"], c["nev"]) and r1.shape == () and int(r1) == c["rank"][2]
        np.testing.assert_array_equal(d1, d[2])
    c = cases[-1]
    d, _, r = obs.gedmd_spectrum(gn.gram(c["x"], c["omega"]), c["omega"], c["a"], 2, tol=0.5)       # rmin: a harsh cutoff still keeps nev
    assert int(r) == 2 and d.shape == (2,)


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_symbol_declared_exported_and_listed():
    ti = pkg()
    hdr = open(os.path.join(ROOT, "include", "ti_hip.h")).read()
    L = ti._lib.lib()
    assert re.search(r"\bint ti_obs_rff_gram\(ti_handle\* h, const float\* values, int64_t stride, int64_t n, const double\* omega, const float\* logw,", hdr)
    assert "typedef struct { int32_t d, p; int64_t n_boot, first; uint64_t seed; } ti_gram_desc;" in hdr
    assert "ti_obs_rff_gram" in ti._lib.ABI_SYMBOLS and hasattr(L, "ti_obs_rff_gram")
    assert C.sizeof(ti._lib.GramDesc) == 32
    assert L.ti_version() == 5


def test_refusals_before_the_device():
    """Every check that needs no device is made before the handle is looked at, so a NULL handle exercises all of them."""
    ti = pkg()
    L = ti._lib.lib()
    x = np.zeros((4, 2), np.float32)
    om = np.ones((2, 3))
    idx = np.zeros((2, 4), np.int32)
    out = np.full((3, 3, 3, 2), 7.0)

    def call(n=4, d=2, p=3, stride=2, n_boot=2, ix=None, n_draw=0, mem=0, v=x, omega=om, desc=True, o=out):
        g = ti._lib.GramDesc(d, p, n_boot, 0, 0)
        vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        rc = L.ti_obs_rff_gram(None, vp(v), stride, n, None if omega is None else omega.ctypes.data_as(C.POINTER(C.c_double)), None,
                               C.byref(g) if desc else None, vp(ix), n_draw, vp(o), mem)
        return rc, ti._lib.last_error()

    bad = om.copy()
    bad[1, 2] = np.inf
    for kw, msg in ((dict(v=None), "NULL buffer"), (dict(omega=None), "NULL buffer"), (dict(desc=False), "NULL buffer"), (dict(o=None), "NULL buffer"),
                    (dict(mem=2), "unknown mem"), (dict(n=0), "n must be"), (dict(n=2 ** 31), "n must be"), (dict(d=0), "d must be"), (dict(d=17), "d must be"),
                    (dict(p=0), "p must be"), (dict(p=129), "p must be"), (dict(stride=1), "stride < d"), (dict(omega=bad), "non-finite omega at entry 5"),
                    (dict(omega=np.full((2, 3), np.nan)), "non-finite omega"), (dict(n_boot=-1), "n_boot"), (dict(n_boot=2 ** 20 + 1), "n_boot"),
                    (dict(n_draw=-1), "n_draw"), (dict(ix=idx, n_draw=0), "idx needs"), (dict(), "NULL handle"), (dict(ix=idx, n_draw=4), "NULL handle")):
        rc, text = call(**kw)
        assert rc == ti._lib.TI_E_ARG and msg in text, (kw, rc, text)
    assert (out == 7.0).all()                                      # nothing was written


def test_python_argument_validation():
    ti = pkg()
    obs = ti.observables
    x = np.zeros(8, np.float32)
    om = np.ones((1, 4))
    for kw, msg in ((dict(omega=np.ones(4)), "omega must be"), (dict(omega=np.ones((17, 4))), "omega must be"), (dict(omega=np.ones((1, 129))), "omega must be"),
                    (dict(omega=np.full((1, 4), np.nan)), "finite"), (dict(n_boot=-1), "n_boot"), (dict(n_boot=1.5), "n_boot"), (dict(n_boot=True), "n_boot"),
                    (dict(values=np.zeros((2, 2, 2), np.float32)), "values must be"), (dict(values=np.zeros(0, np.float32)), "values must be")):
        args = dict(values=x, omega=om)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            obs.rff_gram(**args)

    class Huge:                                                    # only the shape is looked at before the cap refuses
        shape = (2 ** 23 + 1,)
    with pytest.raises(ValueError, match="cap"):
        obs.rff_gram(Huge(), om)
    G = np.eye(4, dtype=np.complex128)
    for kw, msg in ((dict(nev=0), "nev"), (dict(nev=5), "nev"), (dict(nev=1.5), "nev"), (dict(a=np.inf), "finite"), (dict(tol=-1.0), "tol"),
                    (dict(gram=np.eye(3)), "gram must be")):
        args = dict(gram=G, omega=om, a=1.6, nev=2, tol=0.0)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            obs.gedmd_spectrum(**args)
    with pytest.raises(ValueError, match="level"):
        obs.gedmd_generator(x, om, 2, 1.6, level=1.0)
    with pytest.raises(ValueError, match="sigma"):
        obs.sample_rff_gaussian(1, 4, 0.0, 0)
    np.testing.assert_array_equal(obs.sample_rff_gaussian(2, 5, 0.6, 11), np.random.RandomState(11).randn(2, 5) / 0.6)
    assert ti._lib.GRAM_MAX_D == 16 and ti._lib.GRAM_MAX_P == 128 and ti._lib.GRAM_MAX_TABLE == 2 ** 27


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
    for tag, count in NEW_KERNELS.items():
        hits = {n: m for n, m in meta.items() if f"{len(tag)}{tag}" in n}
        assert len(hits) == count, (tag, sorted(hits))
        assert set(hits.values()) == {(0, 0, 0)}, hits


def test_gram_kernels_run_on_the_fp64_matrix_cores(code_objects):
    found = {}
    for co in code_objects:
        for name, insns in isa_rules.kernels(co).items():
            if "obs_gram_kernel" in name:
                found[name] = sum(i.startswith("v_mfma_f64_16x16x4") for i in insns)
    assert len(found) == 8 and all(v >= 16 for v in found.values()), found


def test_recorded_isa_comparison_with_the_parent_build():
    """tools/isa_compare.py PARENT.so THIS.so, recorded: no kernel of the parent differs or is missing (the bootstrap kernel, whose
    draw function moved to a shared header, included); the added ones are the above."""
    text = open(os.path.join(ROOT, "profiles", "gedmd_isa_compare.txt")).read()
    m = re.search(r"(\d+) symbols in \S+; identical in \S+: (\d+); differing: (\d+); missing: (\d+); added: (\d+)", text)
    assert m, text[:400]
    total, same, diff, missing, added = map(int, m.groups())
    assert total == same and diff == 0 and missing == 0
    added_names = re.findall(r"^ADDED (.*)$", text, flags=re.M)
    assert added == len(added_names) == sum(NEW_KERNELS.values())
    for tag in NEW_KERNELS:
        assert any(tag in n for n in added_names), tag
