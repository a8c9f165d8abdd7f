"""gEDMD at the molecule study's size without a GPU: the C ABI of ti_obs_rff_gram_wide (declared, exported, listed, the refusals that
need no device), the argument checks of rff_gram_wide / gedmd_vamp_score / gedmd_cv, the Gram-only restatement of the cross-validated
score (tests/gedmd_wide_numpy.py) and the product's host algebra against the reference (tests/golden/gedmd_wide_reference.npz, written
by tests/golden/make_golden_gedmd_wide.py), the tile bookkeeping of the blocked pass, the code objects of its kernels (no private
segment, no spills), and the drivers' `kinetics` key."""
import ctypes as C
import os
import re
import tempfile
import types

import numpy as np
import pytest

from conftest import ROOT, load_golden, pkg
import gedmd_numpy as gn
import gedmd_wide_numpy as gw
import test_build_isa as isa_rules
from test_edge_mask_host import _kernel_metadata

WIDE_KERNELS = 16                                   # obs_gram_wide_kernel<TJ, DIAG>: TJ = 1..8, on and off the diagonal
SHAPES = [(6, 300, 3000, 4, 1), (6, 300, 3000, 4, 1), (2, 130, 1500, 4, 0), (1, 50, 1000, 4, 0), (1, 16, 257, 4, 0), (6, 513, 2000, 4, 1)]


def fixture_cases():
    """The recorded cases as dicts: x [m, d] fp32, omega [d, p], idx [3, m] (choice rows), perm [3, m] (splits), ev [4, nev], rank [4],
    cv_ev [3, nev], cv_score [3], cv_rank [3]; and (ev_dev, score_dev)"""
    g = load_golden("gedmd_wide_reference")
    cases = []
    for c, (d, p, m, nev, wrap) in enumerate(g["cases"]):
        cut = lambda name, off: g[name][g[off][c]:g[off][c + 1]]
        cases.append(dict(
            name=f"d{d}-p{p}-m{m}-s{g['sigma'][c]:g}", d=int(d), p=int(p), m=int(m), nev=int(nev), a=float(g["a"][c]), tol=float(g["tol"]),
            n_train=int(np.floor(float(g["rtrain"]) * m)), rtrain=float(g["rtrain"]), x=cut("x_flat", "x_off").reshape(m, d),
            omega=cut("omega_flat", "om_off").reshape(d, p), idx=cut("idx_flat", "idx_off").astype(np.int32).reshape(3, m),
            perm=cut("perm_flat", "perm_off").astype(np.int32).reshape(3, m), ev=g["ev"][c][:, :nev], rank=g["rank"][c],
            cv_ev=g["cv_ev"][c][:, :nev], cv_score=g["cv_score"][c], cv_rank=g["cv_rank"][c]))
    return cases, float(g["ev_dev"]), float(g["score_dev"])


# ------------------------------------------------------------------------------------------------------------ the oracle
def test_fixture_is_what_its_script_describes():
    cases, ev_dev, score_dev = fixture_cases()
    g = load_golden("gedmd_wide_reference")
    assert [tuple(int(v) for v in c) for c in g["cases"]] == SHAPES and g["sigma"].tolist() == [5.0, 2.0, 0.6, 0.6, 0.6, 2.0]
    assert 0 < ev_dev < 1e-9 and 0 < score_dev < 1e-9
    for c in cases:
        assert c["x"].dtype == np.float32 and (np.sort(c["perm"], axis=1) == np.arange(c["m"])).all()
        if "s5" in c["name"] or c["p"] == 513:
            assert np.abs(c["x"]).max() <= np.float32(np.pi)                          # the torsion-like cases are wrapped
    assert cases[0]["rank"].max() < 300 and (cases[1]["rank"] == 300).all()          # the cutoff binds at sigma 5, full rank at sigma 2
    assert np.isfinite(np.concatenate([c["cv_score"] for c in cases])).all()


def test_restated_cv_reproduces_the_reference_fixture():
    """Ranks equal; eigenvalues within 64 ev_dev and scores within 64 score_dev: both sides are fp64 LAPACK, the deviations are theirs
    where the fixture was written -- the largest difference seen there, so a bound of 1 x would fail on any other summation order --
    and the factor allows for another BLAS / LAPACK build or thread count (the allowance of tests/test_gedmd_host.py).  Every case,
    p = 300 and 513 included."""
    cases, ev_dev, score_dev = fixture_cases()
    worst = [0.0, 0.0]
    for c in cases:
        for i, row in enumerate([None, *c["idx"]]):
            d, _, r = gn.spectrum(gn.gram(c["x"], c["omega"], row), c["omega"], c["a"], c["nev"], c["tol"])
            assert r == c["rank"][i], (c["name"], i)
            assert np.abs(d - c["ev"][i]).max() <= 64 * ev_dev, (c["name"], i)
        for i, perm in enumerate(c["perm"]):
            d, score, r = gw.cv_split(c["x"], c["omega"], c["a"], c["nev"], c["tol"], perm, c["n_train"])
            worst = [max(worst[0], np.abs(d - c["cv_ev"][i]).max()), max(worst[1], abs(score - c["cv_score"][i]))]
            assert r == c["cv_rank"][i], (c["name"], i)
            assert np.abs(d - c["cv_ev"][i]).max() <= 64 * ev_dev and abs(score - c["cv_score"][i]) <= 64 * score_dev, (c["name"], i)
    print(f"restated cv against the reference: eigenvalues {worst[0]:.2e} (ev_dev {ev_dev:.2e}), scores {worst[1]:.2e} (score_dev {score_dev:.2e})")


def numpy_gram(values, omega, logw=None, n_boot=0, seed=0, first=0, indices=None, engine=None):
    """rff_gram_wide's result from the oracle (explicit indices only)"""
    return gn.gram_rows(values, omega, logw, n_boot, seed, first, indices=indices if indices is not None else [])


def test_product_cv_and_generator_against_the_fixture(monkeypatch):
    """observables.gedmd_cv and gedmd_generator with the GPU Gram call replaced by the oracle's: the host algebra (batched spectrum,
    gedmd_vamp_score, the cut of a permutation into training and held-out indices) on every case, p = 300 and 513 included."""
    obs = pkg().observables
    monkeypatch.setattr(obs, "rff_gram_wide", numpy_gram)
    monkeypatch.setattr(obs, "rff_gram", numpy_gram)
    cases, ev_dev, score_dev = fixture_cases()
    for c in cases:
        cv = obs.gedmd_cv(c["x"], c["omega"], c["a"], c["nev"], c["tol"], rtrain=c["rtrain"], splits=c["perm"])
        assert cv.eigenvalues.shape == (3, c["nev"]) and cv.scores.shape == (3,) and cv.rank.shape == (3,)
        np.testing.assert_array_equal(cv.rank, c["cv_rank"])
        assert np.abs(cv.eigenvalues - c["cv_ev"]).max() <= 64 * ev_dev, c["name"]
        assert np.abs(cv.scores - c["cv_score"]).max() <= 64 * score_dev, c["name"]
        assert (cv.scores <= 0).all()                                                 # the reference function's sign
        res = obs.gedmd_generator(c["x"], c["omega"], c["nev"], c["a"], tol=c["tol"], n_boot=3, indices=c["idx"])
        assert res.rank == c["rank"][0] and np.abs(np.vstack([res.eigenvalues, res.estimates]) - c["ev"]).max() <= 64 * ev_dev, c["name"]


def test_vamp_score_batches_and_flags_a_singular_subspace():
    obs = pkg().observables
    rs = np.random.RandomState(3)
    x, om = rs.randn(300, 2).astype(np.float32), rs.randn(2, 12)
    G = np.stack([gn.gram(x, om, rs.choice(300, 200)) for _ in range(4)]).reshape(2, 2, 12, 12)
    _, W, _ = obs.gedmd_spectrum(G, om, 1.6, 3, 1e-6)
    s = obs.gedmd_vamp_score(G, om, 1.6, W)
    assert s.shape == (2, 2)
    for i in range(2):
        for j in range(2):
            assert abs(s[i, j] - gw.vamp_score(G[i, j], om, 1.6, W[i, j])) <= 1e-12 * abs(s[i, j])
    W0 = W.copy()
    W0[1, 0] = 0.0                                                                   # C = 0: no positive lambda
    s0 = obs.gedmd_vamp_score(G, om, 1.6, W0)
    assert np.isnan(s0[1, 0]) and np.array_equal(np.delete(s0.reshape(-1), 2), np.delete(s.reshape(-1), 2))
    assert obs.gedmd_vamp_score(G[0, 0], om, 1.6, W[0, 0]).shape == ()


def test_model_selection_is_the_double_loop(monkeypatch):
    obs = pkg().observables
    monkeypatch.setattr(obs, "rff_gram_wide", numpy_gram)
    rs = np.random.RandomState(5)
    x = rs.randn(200, 2).astype(np.float32)
    EV, VAMP = obs.gedmd_model_selection(x, [0.8, 1.5], [6, 10, 20], 1.6, 2, tol=1e-6, seed=4, ntest=3)
    assert EV.shape == (2, 3, 3, 2) and VAMP.shape == (2, 3, 3)
    cv = obs.gedmd_cv(x, obs.sample_rff_gaussian(2, 10, 1.5, 4), 1.6, 2, 1e-6, ntest=3, seed=4)
    np.testing.assert_array_equal(EV[1, 1], cv.eigenvalues)
    np.testing.assert_array_equal(VAMP[1, 1], cv.scores)
    prs = np.random.RandomState(4)                                                    # splits=None: RandomState(seed).permutation per row
    perms = np.stack([prs.permutation(200) for _ in range(3)])
    np.testing.assert_array_equal(obs.gedmd_cv(x, obs.sample_rff_gaussian(2, 10, 1.5, 4), 1.6, 2, 1e-6, splits=perms).scores, cv.scores)


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_symbol_declared_exported_and_listed():
    ti = pkg()
    hdr = open(os.path.join(ROOT, "include", "ti_hip.h")).read()
    L = ti._lib.lib()
    assert re.search(r"\bint ti_obs_rff_gram_wide\(ti_handle\* h, const float\* values, int64_t stride, int64_t n, const double\* omega, const float\* logw,\s*"
                     r"const ti_gram_desc\* g, const int32_t\* idx, int64_t n_draw, double\* out, int mem\);", hdr)
    assert "#define TI_GRAM_WIDE_MAX_P 1024" in hdr
    assert "ti_obs_rff_gram_wide" in ti._lib.ABI_SYMBOLS and hasattr(L, "ti_obs_rff_gram_wide")
    assert L.ti_obs_rff_gram_wide.argtypes == L.ti_obs_rff_gram.argtypes
    assert ti._lib.GRAM_WIDE_MAX_P == 1024 and ti._lib.GRAM_MAX_P == 128
    assert L.ti_version() == 5


def test_refusals_before_the_device():
    """The TI_E_ARG table of ti_obs_rff_gram, through the wide entry with a NULL handle: p = 0 and 1025 are refused, p = 129 is not
    refused for its size (it reaches the handle check); out stays untouched."""
    ti = pkg()
    L = ti._lib.lib()
    x = np.zeros((4, 2), np.float32)
    idx = np.zeros((2, 4), np.int32)
    out = np.full(16, 7.0)

    def call(n=4, d=2, p=3, stride=2, n_boot=2, ix=None, n_draw=0, mem=0, v=x, omega=None, no_omega=False, desc=True, o=out):
        om = np.ones((d if d > 0 else 1, max(p, 1))) if omega is None else omega
        g = ti._lib.GramDesc(d, p, n_boot, 0, 0)
        vp = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        rc = L.ti_obs_rff_gram_wide(None, vp(v), stride, n, None if no_omega else om.ctypes.data_as(C.POINTER(C.c_double)), None,
                                    C.byref(g) if desc else None, vp(ix), n_draw, vp(o), mem)
        return rc, ti._lib.last_error()

    bad = np.ones((2, 3))
    bad[1, 2] = np.inf
    for kw, msg in ((dict(v=None), "NULL buffer"), (dict(no_omega=True), "NULL buffer"), (dict(desc=False), "NULL buffer"), (dict(o=None), "NULL buffer"),
                    (dict(mem=2), "unknown mem"), (dict(n=0), "n must be"), (dict(n=2 ** 31), "n must be"), (dict(d=0), "d must be"), (dict(d=17), "d must be"),
                    (dict(p=0), "p must be in 1..1024"), (dict(p=1025), "p must be in 1..1024"), (dict(stride=1), "stride < d"),
                    (dict(omega=bad), "non-finite omega at entry 5"), (dict(n_boot=-1), "n_boot"), (dict(n_boot=2 ** 20 + 1), "n_boot"),
                    (dict(n_draw=-1), "n_draw"), (dict(ix=idx, n_draw=0), "idx needs"), (dict(), "NULL handle"), (dict(ix=idx, n_draw=4), "NULL handle"),
                    (dict(p=129), "NULL handle"), (dict(p=1024), "NULL handle")):
        rc, text = call(**kw)
        assert rc == ti._lib.TI_E_ARG and msg in text, (kw, rc, text)
    assert (out == 7.0).all()                                      # nothing was written


def test_python_argument_validation():
    ti = pkg()
    obs = ti.observables
    x = np.zeros(8, np.float32)
    om = np.ones((1, 4))
    for kw, msg in ((dict(omega=np.ones(4)), "omega must be"), (dict(omega=np.ones((17, 4))), "omega must be"), (dict(omega=np.ones((1, 1025))), "1 <= p <= 1024"),
                    (dict(omega=np.full((1, 4), np.nan)), "finite"), (dict(n_boot=-1), "n_boot"), (dict(n_boot=1.5), "n_boot"), (dict(n_boot=True), "n_boot"),
                    (dict(values=np.zeros((2, 2, 2), np.float32)), "values must be"), (dict(values=np.zeros(0, np.float32)), "values must be")):
        args = dict(values=x, omega=om)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            obs.rff_gram_wide(**args)

    class Huge:                                                    # only the shape is looked at before the cap refuses
        shape = (2 ** 17 + 1,)
    with pytest.raises(ValueError, match="cap"):
        obs.rff_gram_wide(Huge(), np.ones((1, 1024)))
    with pytest.raises(ValueError, match="1 <= p <= 128"):        # the narrow call keeps its limit
        obs.rff_gram(x, np.ones((1, 129)))
    with pytest.raises(ValueError, match="solver='device'"):      # and the device solver its own
        obs.gedmd_generator(x, np.ones((1, 300)), 2, 1.6, solver="device")
    perm = np.arange(8, dtype=np.int32)[None]
    for kw, msg in ((dict(rtrain=0.0), "rtrain"), (dict(rtrain=1.0), "rtrain"), (dict(rtrain=0.05), "empty"), (dict(rtrain=0.5, nev=5), "nev"),
                    (dict(nev=0), "nev"), (dict(nev=1.5), "nev"), (dict(ntest=0), "ntest"), (dict(splits=perm[:, :7]), "splits must be"),
                    (dict(splits=np.zeros((1, 8), np.int32)), "permutation"), (dict(splits=perm[0]), "splits must be")):
        args = dict(values=x, omega=om, a=1.6, nev=2)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            obs.gedmd_cv(**args)
    G, W = np.eye(4, dtype=np.complex128), np.eye(4, 2, dtype=np.complex128)
    for kw, msg in ((dict(gram_test=np.eye(3)), "gram_test must be"), (dict(W=np.eye(3, 2)), "W must be"), (dict(W=np.ones((2, 4, 2))), "W must be"),
                    (dict(omega=np.ones(4)), "omega must be"), (dict(a=np.nan), "finite")):
        args = dict(gram_test=G, omega=om, a=1.6, W=W)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            obs.gedmd_vamp_score(**args)


# ------------------------------------------------------------------------------------------------------------ tile bookkeeping
@pytest.mark.parametrize("T", range(9, 65))
def test_blocked_launches_cover_the_upper_triangle_once(T):
    """The tiles the launches of the blocked pass write, restated (gedmd_wide_numpy.wide_launch_tiles), against a brute-force
    enumeration: every (k, l), k <= l < T, exactly once, at the slot the reduce step reads it from -- its position in the row-major
    list of the upper triangle."""
    brute = {}
    for k in range(T):
        for l in range(k, T):
            brute[(k, l)] = len(brute)
    tiles = gw.wide_launch_tiles(T)
    assert len(tiles) == len(brute) == T * (T + 1) // 2
    assert {(k, l): s for k, l, s in tiles} == brute


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


def test_wide_kernels_exist_without_scratch_or_spills(code_objects):
    meta = {}
    for co in code_objects:
        meta.update(_kernel_metadata(co))
    hits = {n: m for n, m in meta.items() if "20obs_gram_wide_kernel" in n}
    assert len(hits) == WIDE_KERNELS, sorted(hits)
    assert set(hits.values()) == {(0, 0, 0)}, hits


def test_wide_kernels_run_on_the_fp64_matrix_cores(code_objects):
    found = {}
    for co in code_objects:
        for name, insns in isa_rules.kernels(co).items():
            if "obs_gram_wide_kernel" in name:
                found[name] = sum(i.startswith("v_mfma_f64_16x16x4") for i in insns)
    assert len(found) == WIDE_KERNELS and all(v >= 16 for v in found.values()), found
    assert max(found.values()) >= 4 * 4 * 16                       # an 8 x 8 pair: 16 tiles a wave, 4 instructions a tile and K step


def test_recorded_isa_comparison_with_the_parent_build():
    """tools/isa_compare.py PARENT.so THIS.so, recorded: every kernel of the parent is instruction-identical (obs_gram_kernel<1..8>
    included: its inner statement now calls the shared gram_tile_step and compiles to the same instructions); the blocked pass is
    what is added."""
    text = open(os.path.join(ROOT, "profiles", "gedmd_wide_isa_compare.txt")).read()
    m = re.search(r"(\d+) symbols in \S+; identical in \S+: (\d+); differing: (\d+); missing: (\d+); added: (\d+)", text)
    assert m, text[:400]
    total, same, diff, missing, added = map(int, m.groups())
    assert total == same and diff == 0 and missing == 0
    added_names = re.findall(r"^ADDED (.*)$", text, flags=re.M)
    assert added == len(added_names) == WIDE_KERNELS and all("obs_gram_wide_kernel" in n for n in added_names)


# ------------------------------------------------------------------------------------------------------------ the drivers' key
def test_kinetics_key_parsing():
    dr = pkg().drivers
    cfg = types.SimpleNamespace(observables={"descriptors": [["torsion", 0, 1, 2, 3]], "every": 2, "kinetics": {"columns": [0], "temperature": 300.0}})
    assert dr._observe_kw(cfg)["observe"] == {"descriptors": [["torsion", 0, 1, 2, 3]], "every": 2}
    assert dr._kinetics_settings({"descriptors": []}) is None
    assert dr._kinetics_settings(cfg.observables, 1) == {"columns": [0], "p": 300, "sigma": 5.0, "nev": 4, "tol": 1e-4, "n_boot": 1000, "seed": 0,
                                                        "temperature": 300.0}
    ok = {"columns": [1, 2], "temperature": 250}
    for bad in (5, {"columns": [0]}, {"temperature": 300}, {**ok, "q": 1}, {**ok, "p": 0}, {**ok, "p": 1025}, {**ok, "p": 2.5}, {**ok, "nev": True},
                {**ok, "n_boot": 0}, {**ok, "seed": -1}, {**ok, "sigma": 0.0}, {**ok, "tol": -1.0}, {**ok, "temperature": 0.0},
                {**ok, "temperature": float("nan")}, {**ok, "columns": []}, {**ok, "columns": [3]}, {**ok, "columns": [-1]}, {**ok, "columns": [0.5]},
                {**ok, "columns": list(range(17))}, {**ok, "columns": 1}, {**ok, "p": 3, "nev": 4}):
        with pytest.raises(ValueError, match="kinetics"):
            dr._kinetics_settings({"kinetics": bad}, 3)


def test_kinetics_key_adds_three_arrays_and_nothing_else(tmp_path, monkeypatch):
    ti = pkg()
    obs, dr = ti.observables, ti.drivers
    cfg = types.SimpleNamespace(observables={"descriptors": [["rmsd"], ["torsion", 0, 1, 2, 3], ["torsion", 1, 2, 3, 4]], "bins": 4,
                                             "kinetics": {"columns": [1, 2], "p": 7, "nev": 2, "n_boot": 5, "seed": 9, "temperature": 250.0}})
    seen = {}

    def fake_summary(cv, dl, bins=32, engine=None):
        return np.zeros((cv.shape[1], bins)), np.zeros((cv.shape[1], bins + 1)), 3.5

    def fake_generator(values, omega, nev, a, **kw):
        seen.update(values=np.asarray(values), omega=omega, nev=nev, a=a, kw=kw)
        return obs.GedmdResult(np.array([-2.0, 0.0]), np.array([[-2.5, -0.1], [-1.5, 0.1]]), np.zeros((5, 2)), np.zeros((7, 2)), 4)

    monkeypatch.setattr(obs, "end_state_summary", fake_summary)
    monkeypatch.setattr(obs, "gedmd_generator", fake_generator)
    rs = np.random.RandomState(1)
    cvs = [rs.rand(3, 4, 3).astype(np.float32), rs.rand(3, 2, 3).astype(np.float32)]
    dr._write_observables(cfg, str(tmp_path / "with.npz"), cvs, [])
    z = np.load(tmp_path / "with.npz")
    assert sorted(z.files) == ["cv", "edges", "ess", "hist", "kinetics_ci", "kinetics_eigenvalues", "kinetics_rank"]
    np.testing.assert_array_equal(z["kinetics_eigenvalues"], [-2.0, 0.0])
    np.testing.assert_array_equal(z["kinetics_ci"], [[-2.5, -0.1], [-1.5, 0.1]])
    assert int(z["kinetics_rank"]) == 4
    np.testing.assert_array_equal(seen["values"], np.concatenate(cvs, axis=1)[-1][:, 1:3])      # the end-state row, the chosen columns
    assert seen["values"].dtype == np.float32
    np.testing.assert_array_equal(seen["omega"], np.random.RandomState(9).randn(2, 7) / 5.0)
    assert seen["a"] == 0.008314462618 * 250.0 and seen["nev"] == 2
    assert seen["kw"] == dict(tol=1e-4, n_boot=5, seed=9)                                        # unweighted: no logw
    # checked before a rollout: against the descriptor count in the molecule drivers, refused by sample_adw
    dr._check_kinetics(cfg)
    dr._check_kinetics(types.SimpleNamespace())
    dr._check_kinetics(types.SimpleNamespace(observables={"descriptors": [["coord", 0]]}), molecules=False)
    with pytest.raises(ValueError, match="sample_ambient / sample_latent"):
        dr._check_kinetics(cfg, molecules=False)
    with pytest.raises(ValueError, match="sample_ambient / sample_latent"):
        dr.sample_adw(types.SimpleNamespace(observables=cfg.observables, beta0s=[1.0], beta1s=[1.25]), types.SimpleNamespace(dim=1), [])
    typo = types.SimpleNamespace(observables={**cfg.observables, "kinetics": {"columns": [1, 3], "temperature": 250.0}}, data_save_path=str(tmp_path / "none"))
    for driver in (dr.sample_ambient, dr.sample_latent):
        with pytest.raises(ValueError, match="columns"):
            driver(typo, None, None)                                                 # before anything is created or run
    assert not (tmp_path / "none").exists()
    # without the key: today's arrays in today's order, and no call
    del cfg.observables["kinetics"]
    seen.clear()
    dr._write_observables(cfg, str(tmp_path / "without.npz"), cvs, [])
    z0 = np.load(tmp_path / "without.npz")
    assert z0.files == ["cv", "hist", "edges", "ess"] and not seen
    for k in ("cv", "hist", "edges", "ess"):
        np.testing.assert_array_equal(z0[k], z[k])
