"""Per-molecule edge sets without a GPU: the C-ABI entry point ti_painn_set_edge_mask (declared, exported, listed, refuses bad
arguments before any device work), the batch helper split_graph_batch (superset template + mask for the reference's finite-cutoff
batches, today's template for uniform ones), the datasets' per-sample graphs, and the code objects of the masked message kernels
(no more private segment or spills than their unmasked twins; the F = 256 ones keep no SGPR in VGPR lanes)."""
import ctypes
import os
import re
import tempfile
import types

import numpy as np
import pytest

from conftest import ROOT, pkg
import test_build_isa as isa_rules


def _batch(templates, A, atoms=None):
    """Reference-shaped batch (edge_index / edge_type / batch / atoms) of len(templates) molecules, each with its own (src, dst, type)."""
    B = len(templates)
    b = types.SimpleNamespace()
    b.edge_index = np.concatenate([np.stack([np.asarray(s, np.int64), np.asarray(d, np.int64)]) + m * A
                                   for m, (s, d, _) in enumerate(templates)], axis=1)
    b.edge_type = np.concatenate([np.asarray(t, np.int64) for _, _, t in templates])
    b.batch = np.repeat(np.arange(B), A)
    b.atoms = np.tile(np.arange(A), B) if atoms is None else np.asarray(atoms)
    return b


def _radius_templates(A, B, seed=0, keep=0.6):
    d = pkg().data
    x = np.random.RandomState(seed).standard_normal((B, A, 3))
    bi = np.array([list(range(A - 1)) + list(range(1, A)), list(range(1, A)) + list(range(A - 1))])
    bt = np.array([(i % 3) + 1 for i in range(A - 1)] * 2)
    dist = np.linalg.norm(x[:, :, None] - x[:, None, :], axis=-1)
    cutoff = float(np.quantile(dist[:, ~np.eye(A, dtype=bool)], keep))
    return [d.build_edge_template(x[b], cutoff, bi, bt) for b in range(B)]


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_symbol_declared_exported_and_listed():
    ti = pkg()
    hdr = open(os.path.join(ROOT, "include", "ti_hip.h")).read()
    assert re.search(r"int ti_painn_set_edge_mask\(ti_handle\* h, const uint32_t\* mask, int64_t B, int mem\);", hdr)
    assert "ti_painn_set_edge_mask" in ti._lib.ABI_SYMBOLS
    L = ti._lib.lib()
    assert hasattr(L, "ti_painn_set_edge_mask")
    assert L.ti_version() == 5


def test_argument_refusals_before_the_device():
    ti = pkg()
    L = ti._lib.lib()
    m = np.ones((2, 4), np.uint32)
    mp = ctypes.c_void_p(m.ctypes.data)
    # the arguments are checked before the handle, each refusal with its own message, so a NULL handle reaches every branch
    cases = [((None, mp, 2, 0), "not a painn handle"), ((None, None, 0, 0), "not a painn handle"), ((None, mp, 0, 0), "B < 1"),
             ((None, mp, -3, 1), "B < 1"), ((None, mp, 2, 7), "unknown mem"), ((None, None, 0, -1), "unknown mem")]
    for args, msg in cases:
        assert L.ti_painn_set_edge_mask(*args) == ti._lib.TI_E_ARG, args
        assert ti._lib.last_error() == msg, (args, ti._lib.last_error())


# ------------------------------------------------------------------------------------------------------------ batch helper
def test_uniform_batch_gives_todays_template_and_no_mask():
    ti = pkg()
    mol = ti.thermo._molecule
    A = 6
    src, dst, et = ti.synthetic.fully_connected_template(A)
    b = _batch([(src, dst, et)] * 3, A)
    got = mol.split_graph_batch(b, "atoms")
    ref = mol.split_batch(b, "atoms")
    assert got[-1] is None
    for a, r in zip(got[:-1], ref):
        np.testing.assert_array_equal(a, r)


def test_superset_and_mask_of_a_finite_cutoff_batch():
    ti = pkg()
    mol = ti.thermo._molecule
    A, B = 9, 5
    tpls = _radius_templates(A, B)
    assert len({len(t[0]) for t in tpls}) > 1                      # molecules hold different numbers of edges
    Bg, Ag, src, dst, et, ids, mask = mol.split_graph_batch(_batch(tpls, A), "atoms")
    assert (Bg, Ag) == (B, A) and mask.shape == (B, A) and mask.dtype == np.uint32
    s_all, d_all = np.nonzero(~np.eye(A, dtype=bool))
    np.testing.assert_array_equal(src, s_all)
    np.testing.assert_array_equal(dst, d_all)
    np.testing.assert_array_equal(ids, np.arange(A))
    for b, (s, d, t) in enumerate(tpls):
        want = np.zeros(A, np.uint32)
        for s_, d_ in zip(s, d):
            want[d_] |= np.uint32(1) << np.uint32(s_)
        np.testing.assert_array_equal(mask[b], want)
        for s_, d_, t_ in zip(s, d, t):                             # each pair's type is the one the batch shows
            assert et[s_ * (A - 1) + (d_ if d_ < s_ else d_ - 1)] == t_
    # pairs no molecule has: type 0 and masked everywhere
    seen = np.zeros((A, A), bool)
    for s, d, _ in tpls:
        seen[s, d] = True
    for k in range(src.size):
        if not seen[src[k], dst[k]]:
            assert et[k] == 0 and not any((mask[b, dst[k]] >> src[k]) & 1 for b in range(B))
    # the molecules of a radius + bond graph are symmetric
    assert all(((mask[b, :, None] >> np.arange(A)) & 1 == ((mask[b, None, :] >> np.arange(A)[:, None]) & 1)).all() for b in range(B))


def test_edges_are_assigned_by_batch_index_not_by_count():
    """Molecule 0 holds fewer edges than molecule 1: reshaping by E / B would mix them up."""
    ti = pkg()
    A = 4
    t0 = (np.array([0, 1]), np.array([1, 0]), np.array([1, 1]))
    t1 = (np.array([0, 1, 1, 2, 2, 3]), np.array([1, 0, 2, 1, 3, 2]), np.array([1, 1, 0, 0, 0, 0]))
    *_, mask = ti.thermo._molecule.split_graph_batch(_batch([t0, t1], A), "atoms")
    np.testing.assert_array_equal(mask, np.array([[0b10, 0b01, 0, 0], [0b10, 0b101, 0b1010, 0b100]], np.uint32))


def test_refusals_conflicting_types_and_atom_ids():
    ti = pkg()
    mol = ti.thermo._molecule
    A = 4
    t0 = (np.array([0, 1]), np.array([1, 0]), np.array([1, 1]))
    t1 = (np.array([0, 1, 2, 3]), np.array([1, 0, 3, 2]), np.array([2, 2, 0, 0]))      # pair (0, 1) typed 2 here, 1 in molecule 0
    with pytest.raises(ValueError, match="differ"):
        mol.split_graph_batch(_batch([t0, t1], A), "atoms")
    t1 = (np.array([0, 1, 2, 3]), np.array([1, 0, 3, 2]), np.array([1, 1, 0, 0]))
    with pytest.raises(ValueError, match="differ"):
        mol.split_graph_batch(_batch([t0, t1], A, atoms=[0, 1, 2, 3, 0, 1, 3, 2]), "atoms")
    mol.split_graph_batch(_batch([t0, t1], A), "atoms")             # the consistent batch is accepted


def test_asymmetric_masks_are_detected():
    """The pair layout needs symmetric sets: the helper's masks of radius graphs are, a directed edge alone is not."""
    ti = pkg()
    A = 4
    t0 = (np.array([0, 1]), np.array([1, 0]), np.array([0, 0]))
    t1 = (np.array([0, 1, 2]), np.array([1, 0, 3]), np.array([0, 0, 0]))          # 2 -> 3 without 3 -> 2
    *_, mask = ti.thermo._molecule.split_graph_batch(_batch([t0, t1], A), "atoms")
    sym = lambda m: all(((m[d] >> s) & 1) == ((m[s] >> d) & 1) for s in range(A) for d in range(A))
    assert sym(mask[0]) and not sym(mask[1])


# ------------------------------------------------------------------------------------------------------------ datasets
def _traj_file(tmp_path, A=7, n=9, seed=2, spread=None):
    rs = np.random.RandomState(seed)
    traj = rs.standard_normal((8, n, A, 3))
    if spread is not None:
        traj = traj * spread[None, :, None, None]
    os.makedirs(tmp_path / "test", exist_ok=True)
    np.save(tmp_path / "test" / "00031.npy", traj)
    return traj


def test_finite_cutoff_dataset_builds_each_samples_graph(tmp_path):
    ti = pkg()
    d = ti.data
    A = 7
    _traj_file(tmp_path, A=A, spread=np.linspace(0.5, 2.0, 9))
    bi = np.array([[0, 1, 1, 2], [1, 0, 2, 1]])
    bt = np.array([2, 2, 1, 1])
    ds = d.MDQM9SamplerDataset("00031.npy", str(tmp_path), "test", T0=1000, T1=300, scale=False, cutoff=1.2, bond_index=bi, bonds=bt)
    order = np.random.RandomState(0).permutation(len(ds))
    seen_diff = False
    for k, batch in enumerate(ds.batches(4, shuffle=True, seed=0)):
        idx = order[4 * k: 4 * k + 4]
        x0 = batch.x0.reshape(-1, A, 3)
        bidx = batch.batch[batch.edge_index[0]]
        for m, i in enumerate(idx):
            want = d.build_edge_template(x0[m], 1.2, bi, bt)
            sel = bidx == m
            np.testing.assert_array_equal(batch.edge_index[0, sel] - m * A, want[0])
            np.testing.assert_array_equal(batch.edge_index[1, sel] - m * A, want[1])
            np.testing.assert_array_equal(batch.edge_type[sel], want[2])
            seen_diff |= len(want[0]) != len(ds.template[0])
    assert seen_diff                                                 # the cutoff really gives frames different graphs


def test_cutoff_1000_batches_equal_the_single_template(tmp_path):
    ti = pkg()
    d = ti.data
    A = 7
    _traj_file(tmp_path, A=A)
    ds = d.MDQM9SamplerDataset("00031.npy", str(tmp_path), "test", T0=1000, T1=300, scale=True, cutoff=1000)
    for batch in ds.batches(4, shuffle=True, seed=3):
        B = batch.x0.shape[0] // A
        ref = d.make_batch("ambient", batch.x0.reshape(B, A, 3), ds.template, T0=1000, T1=300, atom_ids=ds.atom_ids)
        np.testing.assert_array_equal(batch.edge_index, ref.edge_index)
        np.testing.assert_array_equal(batch.edge_type, ref.edge_type)
        assert ti.thermo._molecule.split_graph_batch(batch, "atoms")[-1] is None


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


def _kernel_metadata(co):
    """{mangled kernel name: (private_segment_fixed_size, sgpr_spill_count, vgpr_spill_count)} from the code object's notes."""
    notes = __import__("subprocess").run([isa_rules._tool("llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    out = {}
    for blk in re.split(r"\n  - \.", notes)[1:]:                       # one entry of amdhsa.kernels each
        m = re.search(r"\n    \.name:\s+(\S+)", blk)
        if not m:
            continue
        name = m.group(1)
        get = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", blk).group(1))
        out[name] = (get("private_segment_fixed_size"), get("sgpr_spill_count"), get("vgpr_spill_count"))
    return out


def test_masked_kernels_spill_no_more_than_their_twins(code_objects):
    meta = {}
    for co in code_objects:
        meta.update(_kernel_metadata(co))
    twins = 0
    for name, m in meta.items():
        for masked_tag, plain_tag in (("painn_edge_mask_kernel", "painn_edge_kernel"), ("painn_pair_mask_kernel", "painn_pair_kernel"),
                                      ("painn_jvp_edge_mask_kernel", "painn_jvp_edge_kernel")):
            if masked_tag not in name:
                continue
            # the twin's mangled name: same template arguments and parameters, the other kernel name (and its length prefix)
            plain_name = name.replace(f"{len(masked_tag)}{masked_tag}", f"{len(plain_tag)}{plain_tag}")
            assert plain_name in meta, (name, plain_name)
            p = meta[plain_name]
            assert m[0] <= p[0] and m[1] <= p[1] and m[2] <= p[2], (name, m, p)
            twins += 1
    assert twins == 172, twins          # directed (128), pair (36) and tangent (8) masked instantiations, one per unmasked kernel


def test_masked_f256_kernels_hold_no_sgpr_in_vgpr_lanes(code_objects):
    guarded = {name: insns for co in code_objects for name, insns in isa_rules.kernels(co).items() if "painn_edge_mask_kernel<16," in name}
    assert len(guarded) == 24, sorted(guarded)
    bad = {k: v for k, v in ((n, isa_rules.lane_spills_outside_scratch(i)) for n, i in guarded.items()) if v}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------ reference graphs
@pytest.mark.parametrize("name", ["mask_ambient", "mask_latent", "mask_ambient_f256", "mask_latent_f256"])
def test_reference_graphs_of_the_golden_batch(name, tmp_path):
    """tests/golden/make_golden_mask.py ran the reference's per-sample AddRadiusGraph / AddBondGraph / Coalesce: the dataset's per-sample
    graphs and split_graph_batch's mask must reproduce them."""
    from conftest import load_golden
    ti = pkg()
    g = load_golden(name)
    A, B = int(g["A"]), int(g["B"])
    ei, et = g["edge_index"], g["edge_type"]
    mol = g["batch"][ei[0]]
    traj = np.zeros((8,) + g["x"].shape)
    traj[7] = g["x"]
    os.makedirs(tmp_path / "test")
    np.save(tmp_path / "test" / "00031.npy", traj)
    ds = ti.data.MDQM9SamplerDataset("00031.npy", str(tmp_path), "test", T0=1000, T1=300, scale=False, cutoff=float(g["cutoff"]),
                                     bond_index=g["bond_index"], bonds=g["bonds"])
    (batch,) = list(ds.batches(B, shuffle=False))
    np.testing.assert_array_equal(batch.edge_index, ei)
    np.testing.assert_array_equal(batch.edge_type, et)
    *_, mask = ti.thermo._molecule.split_graph_batch(types.SimpleNamespace(edge_index=ei, edge_type=et, batch=g["batch"],
                                                                          atoms=g["atom_ids"]), "atoms")
    want = np.zeros((B, A), np.uint32)
    for s, d, m in zip(ei[0] % A, ei[1] % A, mol):
        want[m, d] |= np.uint32(1) << np.uint32(s)
    np.testing.assert_array_equal(mask, want)
    assert want[0][A - 1] == 0                                       # molecule 0's last atom: no incoming edge
