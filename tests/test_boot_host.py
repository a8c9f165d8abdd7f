"""ti_obs_bootstrap without a GPU: the C ABI (declared, exported, listed, the refusals that need no device), the numpy restatement
(tests/boot_numpy.py) against the reference's own bootstrap (tests/golden/boot_reference.npz, written by
tests/golden/make_golden_boot.py), the restated Philox draws (range, uniformity), the argument checks of observables.py, and the code
objects of the new kernels (no private segment, no spills)."""
import ctypes as C
import os
import re
import tempfile

import numpy as np
import pytest

from conftest import ROOT, load_golden, pkg
import boot_numpy as bn
import test_build_isa as isa_rules
from test_edge_mask_host import _kernel_metadata

NEW_KERNELS = ("obs_boot_kernel", "obs_boot_compact_kernel")
EPS = 2.0 ** -53


def fixture_cases():
    """The recorded cases as dicts: logw [n] fp32, idx [n_boot, n_draw] int32 (n_draw may be 0), est [n_boot], and the scalars."""
    g = load_golden("boot_reference")
    cases = []
    for c in range(g["case_data"].size):
        d, nb, nd = int(g["case_data"][c]), int(g["case_n_boot"][c]), int(g["case_n_draw"][c])
        cases.append(dict(
            name=f"{g['names'][d]}-e{int(g['case_estimator'][c])}-m{int(g['case_mode'][c])}-k{g['case_k'][c]:g}",
            logw=g["logw_flat"][g["logw_off"][d]:g["logw_off"][d + 1]], estimator=int(g["case_estimator"][c]), mode=int(g["case_mode"][c]),
            k=float(g["case_k"][c]), n_boot=nb, n_draw=nd, kept=int(g["case_kept"][c]), point=float(g["case_point"][c]),
            lo=float(g["case_lo"][c]), hi=float(g["case_hi"][c]),
            idx=g["idx_flat"][g["idx_off"][c]:g["idx_off"][c + 1]].astype(np.int32).reshape(nb, nd), est=g["est_flat"][g["est_off"][c]:g["est_off"][c + 1]]))
    return cases


def bound(case, ref):
    """8 n_draw 2^-53 (1 + |ref|): the worst case of an n-term positive fp64 sum through a ratio of squares, plus the exp rounding;
    MEAN sums signed terms: 8 n_draw 2^-53 (1 + max |logw|).  The point estimate sums the kept sample: n_draw -> n."""
    scale = np.abs(case["logw"]).max() if case["estimator"] == bn.MEAN else np.abs(ref)
    return 8 * max(case["n_draw"], 1) * EPS * (1 + scale)


def check_against_fixture(case, point, lo, hi, kept, est, worst):
    """kept counts and the NaN pattern exactly, estimates and interval ends within `bound`; worst[0] collects the largest fraction of it"""
    assert kept == case["kept"], case["name"]
    ref = case["est"]
    np.testing.assert_array_equal(np.isnan(est), np.isnan(ref), err_msg=case["name"])
    pairs = [(point, case["point"], 8 * case["logw"].size * EPS * (1 + (np.abs(case["logw"]).max() if case["estimator"] == bn.MEAN else abs(case["point"]))))]
    pairs += [(e, r, bound(case, r)) for e, r in zip(est, ref)] + [(lo, case["lo"], bound(case, case["lo"])), (hi, case["hi"], bound(case, case["hi"]))]
    for got, want, b in pairs:
        assert np.isnan(got) == np.isnan(want), case["name"]
        if not np.isnan(want):
            worst[0] = max(worst[0], abs(got - want) / b)
            assert abs(got - want) <= b, (case["name"], got, want, b)


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_symbol_declared_exported_and_listed():
    ti = pkg()
    hdr = open(os.path.join(ROOT, "include", "ti_hip.h")).read()
    L = ti._lib.lib()
    assert re.search(r"\bint ti_obs_bootstrap\(ti_handle\* h, const float\* logw, int64_t n, const ti_boot_desc\* d,", hdr)
    assert "ti_obs_bootstrap" in ti._lib.ABI_SYMBOLS and hasattr(L, "ti_obs_bootstrap")
    for word in ("TI_BOOT_ESS = 0, TI_BOOT_TFEP = 1, TI_BOOT_MEAN = 2", "TI_BOOT_FILTER_NONE = 0, TI_BOOT_FILTER_ONCE = 1, TI_BOOT_FILTER_RESAMPLE = 2",
                 "0x424f4f54"):
        assert word in hdr, word
    assert ti._lib.BOOT_DOMAIN == bn.DOMAIN == 0x424F4F54
    assert C.sizeof(ti._lib.BootDesc) == 48
    assert L.ti_version() == 5


def test_refusals_before_the_device():
    """Every check that needs no device is made before the handle is looked at, so a NULL handle exercises all of them."""
    ti = pkg()
    L = ti._lib.lib()
    E = ti._lib.TI_E_ARG
    logw = np.zeros(4, np.float32)
    idx = np.zeros((2, 4), np.int32)
    out = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0)

    def call(n=4, est=0, flt=0, k=1.5, level=0.95, n_boot=2, first=0, ix=None, n_draw=0, mem=0, lw=logw, desc=True, o=out):
        d = ti._lib.BootDesc(est, flt, k, level, n_boot, first, 0)
        rc = L.ti_obs_bootstrap(None, None if lw is None else C.c_void_p(lw.ctypes.data), n, C.byref(d) if desc else None,
                                None if ix is None else C.c_void_p(ix.ctypes.data), n_draw, o, None, mem)
        return rc, ti._lib.last_error()

    for kw, msg in ((dict(lw=None), "NULL buffer"), (dict(desc=False), "NULL buffer"), (dict(o=None), "NULL buffer"), (dict(mem=2), "unknown mem"),
                    (dict(n=0), "n must be"), (dict(n=2 ** 31), "n must be"), (dict(est=3), "unknown estimator"), (dict(est=-1), "unknown estimator"),
                    (dict(flt=3), "unknown filter"), (dict(flt=1, k=0.0), "k must be"), (dict(flt=2, k=float("nan")), "k must be"),
                    (dict(flt=1, k=float("inf")), "k must be"), (dict(level=0.0), "level"), (dict(level=1.0), "level"), (dict(level=float("nan")), "level"),
                    (dict(n_boot=-1), "n_boot"), (dict(n_boot=2 ** 20 + 1), "n_boot"), (dict(n_draw=-1), "n_draw"), (dict(ix=idx, n_draw=0), "idx needs"),
                    (dict(), "NULL handle"), (dict(flt=0, k=float("nan")), "NULL handle"), (dict(ix=idx, n_draw=4), "NULL handle")):
        rc, text = call(**kw)
        assert rc == E and msg in text, (kw, rc, text)
    assert list(out) == [7.0] * 4                                  # nothing was written


def test_python_argument_validation():
    ti = pkg()
    obs = ti.observables
    lw = np.zeros(8, np.float32)
    for kw, msg in ((dict(estimator="var"), "estimator"), (dict(estimator="ess", filter="twice", k=2.0), "filter must"),
                    (dict(estimator="ess", filter="once"), "finite k"), (dict(estimator="tfep", k=-1.0), "finite k"),
                    (dict(estimator="ess", n_boot=-1), "n_boot"), (dict(estimator="ess", n_boot=2.5), "n_boot"), (dict(estimator="ess", level=1.0), "level")):
        with pytest.raises(ValueError, match=msg):
            obs.bootstrap(lw, **kw)
    with pytest.raises(ValueError, match="1-D"):
        obs.bootstrap(np.zeros((2, 2), np.float32), "ess")
    # phi is formed in fp64 and rounded once
    E0, E1, dl = np.array([1e8, 3.0]), np.array([1e8 + 0.25, 1.0]), np.array([0.125, -0.5], np.float32)
    np.testing.assert_array_equal(obs._neg_phi(E1, obs._neg(E0), dl), np.array([-0.375, 2.5], np.float32))
    assert obs._neg_phi(E1).dtype == np.float32


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_restatement_reproduces_the_reference_fixture():
    cases = fixture_cases()
    ns = {c["logw"].size for c in cases}
    assert {1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 1000, 4097} <= ns
    assert {(c["estimator"], c["mode"]) for c in cases} == {(e, m) for e in range(3) for m in range(3)}
    assert {c["k"] for c in cases if c["mode"]} == {1.5, 100.0}
    assert all(3 <= c["n_boot"] <= 64 for c in cases)
    assert any(c["mode"] == bn.RESAMPLE and 0 < c["n_draw"] != c["logw"].size for c in cases)       # the reference's draw-count quirk
    assert any(np.isnan(c["est"]).all() for c in cases) and any(np.isnan(c["est"]).any() and not np.isnan(c["est"]).all() for c in cases)
    worst = [0.0]
    for c in cases:
        point, lo, hi, kept, est = bn.bootstrap(c["logw"], c["estimator"], c["mode"], c["k"], 0.95, c["n_boot"], indices=c["idx"] if c["n_draw"] else None)
        check_against_fixture(c, point, lo, hi, kept, est, worst)
    print(f"restatement: worst error {worst[0]:.3f} of the bound")


def test_restated_draws_range_uniformity_and_addressing():
    for n in (1, 2, 3, 64, 1000, 2 ** 31 - 1):
        ix = bn.draws(12345, 7, 513, n)
        assert ix.dtype == np.int32 and ix.shape == (513,) and ix.min() >= 0 and ix.max() < n
    ix = bn.draws(2024, 3, 2 ** 16, 64)
    counts = np.bincount(ix, minlength=64)
    chi2 = ((counts - 1024.0) ** 2 / 1024.0).sum()
    assert chi2 < 63 + 6 * np.sqrt(2 * 63), chi2                   # 63 degrees of freedom, six standard deviations
    # a draw depends on (seed, R, j, n_pop) only: a prefix of a longer row, another row, another seed
    np.testing.assert_array_equal(bn.draws(2024, 3, 101, 64), ix[:101])
    assert (bn.draws(2024, 4, 2 ** 10, 64) != ix[:2 ** 10]).mean() > 0.9
    assert (bn.draws(2025, 3, 2 ** 10, 64) != ix[:2 ** 10]).mean() > 0.9
    assert (bn.draws(2024, 3 + 2 ** 32, 2 ** 10, 64) != ix[:2 ** 10]).mean() > 0.9      # the high word of R enters
    np.testing.assert_array_equal(bn.draw_rows(2024, 2, 3, 50, 64)[1], ix[:50])
    # Philox4x32-10 known answer (Random123 kat_vectors: counter and key all ones)
    o = bn.philox4x32_10(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    assert [int(v) for v in o] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


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
