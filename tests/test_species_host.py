"""Mixed-species batches without a GPU: the C-ABI entry point ti_painn_set_molecules (declared, exported, listed, refuses bad
arguments before any device work), the batch splitter split_species_batch (padded layout, index maps, per-molecule masks and edge
types; a uniform batch takes split_graph_batch's path unchanged), the data helper that concatenates per-species items, and the code
objects: the recorded kernel-by-kernel comparison with the parent build (profiles/species_isa_compare.txt: every pre-existing kernel
symbol instruction-identical) and the new integrator / pad kernels (no private segment, no spills)."""
import ctypes
import os
import re
import tempfile
import types

import numpy as np
import pytest

from conftest import ROOT, pkg
import test_build_isa as isa_rules
from test_edge_mask_host import _kernel_metadata

SIZES = (5, 9, 12)


def _species_items(per=2, seed=0):
    """Per-species sampler items (data.make_batch) of three species with A = 5, 9, 12: a radius graph per molecule plus chain bonds
    whose orders differ from species to species."""
    d = pkg().data
    items, tpls = [], []
    for k, A in enumerate(SIZES):
        rs = np.random.RandomState(seed + A)
        x = rs.standard_normal((per, A, 3)).astype(np.float32)
        x -= x.mean(axis=1, keepdims=True)
        bi = np.array([list(range(A - 1)) + list(range(1, A)), list(range(1, A)) + list(range(A - 1))])
        bt = np.array([((i + k) % 3) + 1 for i in range(A - 1)] * 2)
        dist = np.linalg.norm(x[:, :, None] - x[:, None, :], axis=-1)
        cutoff = float(np.quantile(dist[:, ~np.eye(A, dtype=bool)], 0.6))
        t = [d.build_edge_template(x[m], cutoff, bi, bt) for m in range(per)]
        tpls += t
        items.append(d.make_batch("ambient", x, t, T0=1000, T1=300 + 100 * k))
    return items, tpls


# ------------------------------------------------------------------------------------------------------------ C ABI
def test_symbol_declared_exported_and_listed():
    ti = pkg()
    hdr = open(os.path.join(ROOT, "include", "ti_hip.h")).read()
    assert re.search(r"int ti_painn_set_molecules\(ti_handle\* h, const int32_t\* n_atoms, const uint32_t\* mask, const uint8_t\* pair_type, "
                     r"int64_t B, int mem\);", hdr)
    assert "ti_painn_set_molecules" in ti._lib.ABI_SYMBOLS
    L = ti._lib.lib()
    assert hasattr(L, "ti_painn_set_molecules")
    assert L.ti_version() == 5


def test_argument_refusals_before_the_device():
    ti = pkg()
    L = ti._lib.lib()
    n = np.array([3, 4], np.int32)
    p = ctypes.c_void_p(n.ctypes.data)
    cases = [((None, p, None, None, 2, 0), "not a painn handle"), ((None, None, None, None, 0, 0), "not a painn handle"),
             ((None, p, None, None, 0, 0), "B < 1"), ((None, p, None, None, -1, 1), "B < 1"), ((None, p, None, None, 2, 5), "unknown mem")]
    for args, msg in cases:
        assert L.ti_painn_set_molecules(*args) == ti._lib.TI_E_ARG, args
        assert ti._lib.last_error() == msg, (args, ti._lib.last_error())


# ------------------------------------------------------------------------------------------------------------ splitter
def test_mixed_batch_layout_masks_types_and_index_maps():
    ti = pkg()
    mol = ti.thermo._molecule
    items, tpls = _species_items()
    batch = ti.data.concat_species_batches(items)
    N, B, A = sum(2 * a for a in SIZES), 6, max(SIZES)
    assert batch.x0.shape == (N, 3) and batch.batch.max() == B - 1
    with pytest.raises(ValueError):
        mol.split_graph_batch(batch, "atoms")                       # today's splitter refuses unequal molecules
    sb = mol.split_species_batch(batch, "atoms")
    assert (sb.B, sb.A) == (B, A)
    np.testing.assert_array_equal(sb.n_atoms, np.repeat(SIZES, 2))
    np.testing.assert_array_equal(sb.atom_ids, np.arange(A))
    s_all, d_all = np.nonzero(~np.eye(A, dtype=bool))
    np.testing.assert_array_equal(sb.src, s_all)
    np.testing.assert_array_equal(sb.dst, d_all)
    # index maps round-trip: flat -> padded -> flat, and padded positions no node maps to are the pads
    xp = sb.pad(batch.x0, 3)
    assert xp.shape == (B, A, 3)
    np.testing.assert_array_equal(sb.unpad(xp), batch.x0)
    np.testing.assert_array_equal(sb.unpad(np.stack([xp, 2 * xp])), np.stack([batch.x0, 2 * batch.x0]))
    is_pad = np.ones(B * A, bool)
    is_pad[sb.node_index] = False
    np.testing.assert_array_equal(is_pad.reshape(B, A), np.arange(A)[None, :] >= sb.n_atoms[:, None])
    assert (xp.reshape(B * A, 3)[is_pad] == 0).all()
    # masks and types of every molecule; pads have no bits, neither as destination nor as source
    for b, (s, d, t) in enumerate(tpls):
        want = np.zeros(A, np.uint32)
        for s_, d_ in zip(s, d):
            want[d_] |= np.uint32(1) << np.uint32(s_)
        np.testing.assert_array_equal(sb.mask[b], want)
        np.testing.assert_array_equal(sb.pair_type[b][s, d], t)
        n = sb.n_atoms[b]
        assert (sb.mask[b, n:] == 0).all() and (sb.mask[b] >> np.uint32(n) == 0).all()
    assert len({tuple(sb.pair_type[b, 0, 1:3]) for b in (0, 2, 4)}) > 1      # the species really differ in bond types
    # per-node conditioning and times pad to [B, A]
    T1 = sb.pad(batch.T1, 1)[:, :, 0]
    np.testing.assert_array_equal(T1[:, 0], np.repeat([300, 400, 500], 2))
    tv = sb.molecule_values(np.repeat(np.arange(B, dtype=np.float32), sb.n_atoms))
    np.testing.assert_array_equal(tv.reshape(B, A), np.repeat(np.arange(B, dtype=np.float32), A).reshape(B, A))


def test_uniform_batch_yields_exactly_split_graph_batch():
    ti = pkg()
    mol = ti.thermo._molecule
    for tpl_list in (False, True):
        items, tpls = _species_items()
        batch = items[1]                                             # one species: uniform size, per-molecule radius graphs
        if not tpl_list:
            A = SIZES[1]
            src, dst, et = ti.synthetic.fully_connected_template(A)
            batch = ti.data.make_batch("ambient", batch.x0.reshape(2, A, 3), (src, dst, et), T0=1000, T1=300)
        ref = mol.split_graph_batch(batch, "atoms")
        sb = mol.split_species_batch(batch, "atoms")
        assert sb.n_atoms is None and sb.pair_type is None
        for a, r in zip(sb.template(), ref):
            if r is None:
                assert a is None
            else:
                np.testing.assert_array_equal(a, r)
        np.testing.assert_array_equal(sb.node_index, np.arange(batch.x0.shape[0]))
        np.testing.assert_array_equal(sb.unpad(sb.pad(batch.x0, 3)), batch.x0)


def test_refusals_of_the_splitter():
    ti = pkg()
    mol = ti.thermo._molecule
    items, _ = _species_items()
    batch = ti.data.concat_species_batches(items)
    bad = types.SimpleNamespace(**vars(batch))
    bad.atoms = batch.atoms.copy()
    bad.atoms[[0, 1]] = bad.atoms[[1, 0]]
    with pytest.raises(ValueError, match="atom ids"):
        mol.split_species_batch(bad, "atoms")
    bad = types.SimpleNamespace(**vars(batch))
    bad.edge_index = batch.edge_index.copy()
    bad.edge_index[1, 0] = batch.x0.shape[0] - 1
    with pytest.raises(ValueError, match="cross"):
        mol.split_species_batch(bad, "atoms")


def test_engine_set_molecules_checks_shapes_before_the_library():
    ti = pkg()
    eng = ti.engine.PainnEngine.__new__(ti.engine.PainnEngine)      # no handle: the checks below come first
    eng.A, eng.h = 4, None
    with pytest.raises(ValueError, match="mask must be"):
        eng.set_molecules([2, 4], mask=np.zeros((2, 3), np.uint32))
    with pytest.raises(ValueError, match="pair_type must be"):
        eng.set_molecules([2, 4], pair_type=np.zeros((2, 4), np.uint8))
    with pytest.raises(ValueError, match="0..3"):
        eng.set_molecules([2, 4], pair_type=np.full((2, 4, 4), 4))
    with pytest.raises(ti._lib.TiError, match="not a painn handle"):
        eng.set_molecules([2, 4])


# ------------------------------------------------------------------------------------------------------------ the edge-size problem
def test_edge_problem_of_the_gpu_suite_holds_on_its_own():
    """What tests/test_gpu_species_edges.py relies on, checked without a GPU: five kinds whose 3n straddle lane 64; the one-atom kind has no
    edge and its fp64 drift, tangent and divergence are exactly 0 (refs() asserts it); pads carry no mask bit; the restatement of
    per-trajectory dopri5 with dlogp finishes on it (zero drift: the 1e-6 initial step, tenfold growth) with other attempts than a
    kind that moves; the chunk budget's bounds."""
    import test_gpu_species_edges as E
    ks, _ = E.kinds()
    assert [3 * q.n for q in ks] == [3, 6, 63, 66, 75] and not ks[0].on.any()
    assert all((q.on == q.on.T).all() and (q.pt == q.pt.T).all() for q in ks)      # symmetric: the pair layout is eligible
    for what in ("drift", "jvp", "div"):
        assert len(E.refs(what)) == 5
    m = E.mix(261, "far")
    assert (m.x[~m.real] == -1e4).all() and (m.mask[~m.real] == 0).all() and (m.mask >> m.n_atoms[:, None].astype(np.uint32) == 0).all()
    assert (np.bincount(m.kind) >= 52).all() and m.kind[256] != m.kind[0]
    path0, dl0, att0 = E.traj_ref(0, True, False)
    assert (path0 == 0).all() and (dl0 == 0).all() and att0 == 7                   # 44 evaluations
    assert E.traj_ref(1, True, False)[2] != att0
    assert 0.001 <= float(E._budget_gb(4)) < float(E._budget_gb(75))


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


NEW_KERNELS = ("rk_ratio_partial_ragged_kernel", "scaled_sq_partial_ragged_kernel", "traj_init_ragged_kernel", "traj_stage_ragged_kernel",
               "traj_advance_ragged_kernel", "reduce_partials_ragged_kernel", "park_pads_kernel", "zero_pads_kernel", "copy_pads_kernel", "noise_ragged_kernel",
               "div_reduce_ragged_kernel")


def test_new_kernels_exist_without_scratch_or_spills(code_objects):
    meta = {}
    for co in code_objects:
        meta.update(_kernel_metadata(co))
    # the masked twin of the tangent filter pass: no more private segment or spills than its unmasked twin, one per instantiation
    masked_tag, plain_tag = "painn_jvp_filter_mask_kernel", "painn_jvp_filter_kernel"
    twins = [n for n in meta if f"{len(masked_tag)}{masked_tag}" in n]
    assert len(twins) == 8, twins
    for n in twins:
        m, q = meta[n], meta[n.replace(f"{len(masked_tag)}{masked_tag}", f"{len(plain_tag)}{plain_tag}")]
        assert m[0] <= q[0] and m[1] <= q[1] and m[2] <= q[2], (n, m, q)
    for tag in NEW_KERNELS:
        hits = {n: m for n, m in meta.items() if f"{len(tag)}{tag}" in n}
        assert len(hits) == 1, (tag, sorted(hits))
        assert list(hits.values())[0] == (0, 0, 0), hits


def test_recorded_isa_comparison_with_the_parent_build():
    """tools/isa_compare.py PARENT.so THIS.so, recorded like profiles/edge_mask_isa_compare.txt: no kernel of the parent differs or is
    missing, and what the build adds are the kernels above."""
    text = open(os.path.join(ROOT, "profiles", "species_isa_compare.txt")).read()
    m = re.search(r"(\d+) symbols in \S+; identical in \S+: (\d+); differing: (\d+); missing: (\d+); added: (\d+)", text)
    assert m, text[:400]
    total, same, diff, missing, added = map(int, m.groups())
    assert total == same and diff == 0 and missing == 0
    assert "DIFFERS" not in text and "MISSING" not in text
    added_names = re.findall(r"^ADDED (.*)$", text, flags=re.M)
    assert added == len(added_names)
    tags = NEW_KERNELS + ("painn_jvp_filter_mask_kernel",)           # the tangent filter pass on per-molecule row words (edge types)
    for tag in tags:
        assert any(tag in n for n in added_names), tag
    assert all(any(tag in n for tag in tags) for n in added_names), added_names
