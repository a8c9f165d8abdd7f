"""Z-matrix coordinates without a GPU: the fp64 restatement (tests/zmat_numpy.py) against the reference's own functions
(tests/golden/zmat_reference.npz, written by tests/golden/make_golden_zmat.py), its round trip, ZMatrix.from_bonds and every refusal
of ZMatrix, iqr_keep against the reference's filter_iqr, the C ABI (declared, exported, listed, refusals before any device work), the
code objects of the new kernels (no private segment, no spills), the recorded ISA comparison, and the driver key's refusals, which
come before any rollout."""
import os
import re
import tempfile
import types

import numpy as np
import pytest

from conftest import ROOT, load_golden, pkg
import zmat_numpy as zn
import test_build_isa as isa_rules
from test_edge_mask_host import _kernel_metadata

NEW_SYMBOLS = ("ti_obs_zmat", "ti_obs_zmat_xyz", "ti_obs_hist_cols")
NEW_KERNELS = ("obs_zmat_kernel", "obs_zmat_xyz_kernel", "obs_whist_cols_kernel", "obs_keep_max_kernel", "obs_keep_sum_kernel",
               "obs_cols_combine_kernel")


def cases():
    g = load_golden("zmat_reference")
    return [{k[len(f"c{i}_"):]: v for k, v in g.items() if k.startswith(f"c{i}_")} | {"A": int(A)} for i, A in enumerate(g["cases"])]


# ------------------------------------------------------------------------------------------------------------ the oracle
def test_restatement_reproduces_the_reference_fixture():
    """within the e_ref the generator recorded (the reference computes in fp32); the fixture covers what it is there for"""
    cs = cases()
    assert sorted({c["A"] for c in cs}) == [4, 5, 18, 25]
    assert {int(c["ref"][2][0]) for c in cs} == {0, 1}
    for c in cs:
        A, order, ref = c["A"], c["order"], c["ref"]
        assert c["x"].shape == (64, A, 3) and c["x"].dtype == np.float32 and not (order == np.arange(A)).all()
        o2, r2 = zn.from_bonds(c["bonds"], A, int(c["root"]))
        np.testing.assert_array_equal(o2, order); np.testing.assert_array_equal(r2, ref)
        e_z, e_x, e_ld = c["e_ref"]
        assert e_z <= 1e-3 and e_x <= 1e-3 * (1 + np.abs(c["x_ref"]).max()) and e_ld <= 1e-3 * (1 + np.abs(c["logdet_ref"]).max())
        z = zn.construct(c["x"], order, ref)
        assert np.abs(z - c["z_ref"]).max() <= e_z
        assert (z[:, 0, 1:] == 0).all() and (z[:, 1, 2] == 0).all() and (c["z_ref"][:, 0, 1:] == 0).all()
        x, logdet, _, cond = zn.deconstruct(c["z_in"], order, ref)
        assert np.abs(x - c["x_ref"]).max() <= e_x
        assert np.abs(logdet - c["logdet_ref"]).max() <= e_ld and np.abs(logdet - c["logdet2_ref"]).max() <= e_ld
        assert cond.min() >= 0.05 and np.sin(c["z_in"][:, 1:, 1].astype(np.float64)).min() >= 0.3
    g = load_golden("zmat_reference")
    np.testing.assert_array_equal(zn.valid_mask(g["valid_z"]), g["valid_mask"])
    assert g["valid_mask"].tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1]         # a = pi32 and t = +pi32 pass, t = -pi32, NaN, d = 0 do not


def test_restatement_round_trip():
    """z -> x -> z in fp64: the internal coordinates come back to round-off, the structural zeros exactly"""
    for c in cases():
        z0 = c["z_in"].astype(np.float64)
        x, _, _, _ = zn.deconstruct(z0, c["order"], c["ref"])
        z1 = zn.construct(x, c["order"], c["ref"])
        assert np.abs(z1 - z0).max() < 1e-11, c["A"]
        x2, _, _, _ = zn.deconstruct(z1, c["order"], c["ref"])
        assert np.abs(x2 - x).max() < 1e-10


# ------------------------------------------------------------------------------------------------------------ topology
def test_from_bonds_chain_star_ring():
    ZM = pkg().zmatrix.ZMatrix
    chain = ZM.from_bonds([[0, 1], [1, 2], [2, 3], [3, 4]], 5)
    np.testing.assert_array_equal(chain.order, [0, 1, 2, 3, 4])
    np.testing.assert_array_equal(chain.ref, [[0, 0, 0], [0, 0, 0], [1, 0, 0], [2, 1, 0], [3, 2, 1]])
    # from the far end the visit order reverses; the references are in SORTED numbering and look the same
    rev = ZM.from_bonds([[0, 1], [1, 2], [2, 3], [3, 4]], 5, root=4)
    np.testing.assert_array_equal(rev.order, [4, 3, 2, 1, 0])
    np.testing.assert_array_equal(rev.ref, chain.ref)
    star = ZM.from_bonds([[2, 0], [2, 4], [2, 1], [2, 3]], 5, root=2)
    np.testing.assert_array_equal(star.order, [2, 0, 1, 3, 4])
    np.testing.assert_array_equal(star.ref, [[0, 0, 0], [0, 0, 0], [0, 1, 0], [0, 1, 2], [0, 1, 2]])
    # a ring 0-1-2-3-4-0 with a tail 2-5: the closing bond 4-0 makes 4 a child of the root
    ring = ZM.from_bonds([[0, 1], [1, 2], [2, 3], [3, 4], [4, 0], [2, 5]], 6)
    np.testing.assert_array_equal(ring.order, [0, 1, 4, 2, 3, 5])
    np.testing.assert_array_equal(ring.ref, [[0, 0, 0], [0, 0, 0], [0, 1, 0], [1, 0, 2], [2, 0, 1], [3, 1, 0]])
    for zm, bonds, root in ((chain, [[0, 1], [1, 2], [2, 3], [3, 4]], 0), (star, [[2, 0], [2, 4], [2, 1], [2, 3]], 2),
                            (ring, [[0, 1], [1, 2], [2, 3], [3, 4], [4, 0], [2, 5]], 0)):
        o, r = zn.from_bonds(bonds, zm.A, root)
        np.testing.assert_array_equal(o, zm.order); np.testing.assert_array_equal(r, zm.ref)
    assert chain.n_internal == 9 and ZM(None, [[0, 0, 0], [0, 0, 0]]).n_internal == 1
    d = chain.descriptors()
    assert d[0] == ("dist", 1, 0) and d[1] is None and d[2] is None and d[4] == ("angle", 2, 1, 0) and d[8] == ("torsion", 0, 1, 2, 3)
    for bad, msg in ((dict(bonds=[[0, 1], [2, 3]], A=4), "connect"), (dict(bonds=[[0, 1], [1, 1]], A=2), "different"),
                     (dict(bonds=[[0, 4]], A=3), "different atoms of 0..2"), (dict(bonds=[[0, 1]], A=2, root=2), "root"),
                     (dict(bonds=[[0, 1]], A=1), "2 <= A"), (dict(bonds=[[0.5, 1]], A=2), "integer"), (dict(bonds=[0, 1], A=2), "integer array")):
        with pytest.raises(ValueError, match=msg):
            ZM.from_bonds(**bad)


def test_every_zmatrix_refusal():
    zmod = pkg().zmatrix
    good = [[0, 0, 0], [0, 0, 0], [1, 0, 0], [2, 1, 0]]
    zm = zmod.ZMatrix([3, 1, 0, 2], good)
    assert zm.order.dtype == zm.ref.dtype == np.int32 and zm.A == 4
    # unread slots may hold anything and come back as 0
    np.testing.assert_array_equal(zmod.ZMatrix(None, [[9, 9, 9], [0, -7, 99], [1, 0, 55], [2, 1, 0]]).ref, good)
    bad_refs = [([[0, 0, 0], [1, 0, 0], [1, 0, 0], [2, 1, 0]], "ref_atoms.1..0. = 1 is not an earlier"),        # itself
                ([[0, 0, 0], [0, 0, 0], [1, 2, 0], [2, 1, 0]], "ref_atoms.2..1. = 2"),
                ([[0, 0, 0], [0, 0, 0], [1, 1, 0], [2, 1, 0]], "repeats atom 1"),
                ([[0, 0, 0], [0, 0, 0], [1, 0, 0], [2, 1, 2]], "repeats atom 2"),
                ([[0, 0, 0], [0, 0, 0], [1, 0, 0], [2, 1, -1]], "ref_atoms.3..2. = -1"),
                ([[0, 0, 0], [0, 0, 0], [1, 0, 0], [2, 1, 3]], "ref_atoms.3..2. = 3"),
                ([[0, 0], [0, 0]], "integer array .A, 3."), ([[0.0, 0, 0], [0, 0, 0]], "integer array"), ([[0, 0, 0]], "2 <= A <= 32"),
                (np.zeros((33, 3), np.int64), "2 <= A <= 32")]
    for ref, msg in bad_refs:
        with pytest.raises(ValueError, match=msg):
            zmod.ZMatrix(None, ref)
    for order in ([0, 1, 2], [0, 1, 2, 2], [0, 1, 2, 4], [-1, 0, 1, 2], [0.0, 1.0, 2.0, 3.0], [[0, 1, 2, 3]]):
        with pytest.raises(ValueError, match="permutation"):
            zmod.ZMatrix(order, good)
    with pytest.raises(ValueError, match="A = 5 rows"):
        zmod.check_topology(None, good, A=5)
    # the engine checks the species size before the library is reached
    eng = pkg().engine.PainnEngine.__new__(pkg().engine.PainnEngine)
    eng.A, eng.h = 5, None
    with pytest.raises(ValueError, match="A = 4 atoms"):
        eng.zmatrix(np.zeros((2, 5, 3), np.float32), zm)
    eng.A = 4
    with pytest.raises(ValueError, match=r"z must be \[B,3,3\]"):
        eng.zmatrix_xyz(np.zeros((2, 4, 3), np.float32), zm)
    with pytest.raises(TypeError, match="ZMatrix"):
        zmod.zmatrix(eng, np.zeros((2, 4, 3), np.float32), "chain")
    # slices: the reference's gen_torsions / gen_bond_angles / gen_bond_lengths
    z = np.arange(2 * 4 * 3, dtype=np.float32).reshape(2, 4, 3)
    np.testing.assert_array_equal(zmod.torsions(z), z[:, 2:, 2]); np.testing.assert_array_equal(zmod.bond_angles(z), z[:, 1:, 1])
    np.testing.assert_array_equal(zmod.bond_lengths(z), z[:, :, 0])
    np.testing.assert_array_equal(zmod.marginal_columns(5), [0, 3, 6, 9, 4, 7, 10, 8, 11])
    with pytest.raises(ValueError, match=r"z must be \[B, A-1, 3\]"):
        zmod.zmatrix_marginals(np.zeros((4, 6), np.float32))
    with pytest.raises(ValueError, match="bins"):
        zmod.zmatrix_marginals(np.zeros((4, 2, 3), np.float32), bins=300)


def test_iqr_keep_is_the_references_filter():
    g = load_golden("zmat_reference")
    zmod = pkg().zmatrix
    for k, want in zip(g["iqr_k"], g["iqr_keep"]):
        got = zmod.iqr_keep(g["iqr_logw"], float(k))
        assert got.dtype == np.uint8
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(zn.iqr_keep(g["iqr_logw"], float(k)), want)
    assert zmod.iqr_keep(g["iqr_logw"], None).all()
    for bad in (0.0, -1.0, np.nan, True):
        with pytest.raises(ValueError, match="k must be"):
            zmod.iqr_keep(g["iqr_logw"], bad)
    with pytest.raises(ValueError, match="non-finite logw at index 2"):
        zmod.iqr_keep(np.array([0.0, 1.0, np.inf]), 1.5)


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_symbols_declared_exported_and_listed():
    ti = pkg()
    hdr = open(os.path.join(ROOT, "include", "ti_hip.h")).read()
    L = ti._lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(ti_handle\* h, ", hdr), name
        assert name in ti._lib.ABI_SYMBOLS and hasattr(L, name), name
    assert L.ti_version() == 5
    assert (ti._lib.ZMAT_MIN_ATOMS, ti._lib.ZMAT_MAX_ATOMS, ti._lib.HIST_COLS_MAX) == (2, 32, 128)


def test_refusals_before_the_device():
    ti = pkg()
    L = ti._lib.lib()
    E = ti._lib.TI_E_ARG
    assert L.ti_obs_zmat(None, None, None, None, 1, None, 0) == E
    assert ti._lib.last_error() == "not a painn handle"
    assert L.ti_obs_zmat_xyz(None, None, None, None, 1, None, None, None, 0) == E
    assert L.ti_obs_hist_cols(None, None, 1, None, None, 1, 4, None, None, None, None, 0) == E
    assert ti._lib.last_error() == "NULL handle"


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
    text = open(os.path.join(ROOT, "profiles", "zmat_isa_compare.txt")).read()
    m = re.search(r"(\d+) symbols in \S+; identical in \S+: (\d+); differing: (\d+); missing: (\d+); added: (\d+)", text)
    assert m, text[:400]
    total, same, diff, missing, added = map(int, m.groups())
    assert total == same and diff == 0 and missing == 0
    added_names = re.findall(r"^ADDED (.*)$", text, flags=re.M)
    assert added == len(added_names) == len(NEW_KERNELS)
    for tag in NEW_KERNELS:
        assert any(tag in n for n in added_names), tag


# ------------------------------------------------------------------------------------------------------------ the driver key
class _Untouchable:
    """A model stand-in: any use of it means the driver went past its checks"""
    def __getattr__(self, name):
        raise AssertionError(f"the driver touched the model ({name}) before refusing the key")


GOOD_REF = [[0, 0, 0], [0, 0, 0], [1, 0, 0], [2, 1, 0]]


@pytest.mark.parametrize("key, msg", [
    (5, "must be a dict"), ({"ref_atoms": GOOD_REF, "bin": 8}, "keys out of"), ({"bins": 8}, "either 'ref_atoms'"),
    ({"ref_atoms": GOOD_REF, "bonds": [[0, 1]]}, "either 'ref_atoms'"), ({"bonds": [[0, 1]], "order": [0, 1]}, "either 'ref_atoms'"),
    ({"ref_atoms": GOOD_REF, "root": 0}, "either 'ref_atoms'"),
    ({"ref_atoms": [[0, 0, 0], [0, 0, 0], [1, 1, 0]]}, "repeats atom 1"), ({"ref_atoms": GOOD_REF, "order": [0, 1, 2, 2]}, "permutation"),
    ({"bonds": [[0, 1], [2, 3]]}, "connect"), ({"bonds": []}, "non-empty"), ({"bonds": [[0, 1]], "root": 5}, "root"),
    ({"ref_atoms": GOOD_REF, "bins": 0}, "bins"), ({"ref_atoms": GOOD_REF, "length_range": [2.0, 1.0]}, "range"),
    ({"ref_atoms": GOOD_REF, "scale": 0.0}, "scale"), ({"ref_atoms": GOOD_REF, "iqr_k": -1.0}, "iqr_k"),
    ({"ref_atoms": GOOD_REF, "iqr_k": 100.0}, "needs observables.'energy'."),
])
def test_driver_refuses_a_malformed_key_before_any_rollout(key, msg, tmp_path):
    ti = pkg()
    cfg = types.SimpleNamespace(observables={"descriptors": [["dist", 0, 1]], "zmatrix": key}, data_save_path=str(tmp_path / "out"),
                                data_save_name="z", return_dlogp=1)
    with pytest.raises(ValueError, match=r"observables\['zmatrix'\].*" + msg):
        ti.drivers.sample_ambient(cfg, _Untouchable(), _Untouchable())
    assert not os.path.exists(tmp_path / "out")


def test_other_drivers_refuse_the_key_and_the_integrator_never_sees_it():
    ti = pkg()
    cfg = types.SimpleNamespace(observables={"descriptors": [["dist", 0, 1]], "zmatrix": {"ref_atoms": GOOD_REF}}, beta0s=[1.0], beta1s=[1.25])
    with pytest.raises(ValueError, match="is for sample_ambient"):
        ti.drivers.sample_latent(cfg, _Untouchable(), _Untouchable())
    with pytest.raises(ValueError, match="is for sample_ambient"):
        ti.drivers.sample_adw(cfg, types.SimpleNamespace(dim=1), _Untouchable())
    assert ti.drivers._observe_kw(cfg)["observe"] == {"descriptors": [["dist", 0, 1]]}
    g = ti.drivers._check_zmatrix(types.SimpleNamespace(observables={"zmatrix": {"bonds": [[0, 1], [1, 2]], "bins": 8, "scale": 0.5},
                                                                     "energy": {"forcefield": "x", "scale": 0.25}}))
    assert g["zm"].A == 3 and g["bins"] == 8 and g["length_range"] == (0.0, 4.0) and g["scale"] == 0.5 and g["iqr_k"] is None
    g = ti.drivers._check_zmatrix(types.SimpleNamespace(observables={"zmatrix": {"ref_atoms": GOOD_REF, "iqr_k": 100},
                                                                     "energy": {"forcefield": "x", "scale": 0.25}}))
    assert g["scale"] == 0.25 and g["iqr_k"] == 100.0 and g["bins"] == 64
    assert ti.drivers._check_zmatrix(types.SimpleNamespace(observables={"descriptors": []})) is None
    assert ti.drivers._check_zmatrix(types.SimpleNamespace()) is None
