"""ti_obs_zmat / ti_obs_zmat_xyz / ti_obs_hist_cols on the GPU against the fp64 numpy restatement (tests/zmat_numpy.py), ti_obs_cv and
ti_obs_hist (bit for bit), and the reference fixture (tests/golden/zmat_reference.npz).

Bounds.  z: the project's CV bound 1e-6 (1 + |ref|).  Coordinates: 1e-6 (1 + max |coord| of the molecule).  log|det J|:
8 * 3A * 2^-53 (1 + sum |terms|).  Against the fixture the generator's e_ref (the reference's own fp32 error on that case) is added.
Round trip: the ti_obs_cv RMSD between x and zmat_xyz(zmat(x)) is at most twice the restatement's (with z rounded to fp32, as the
device hands it over) plus 1e-6 * scale; the factor 2 covers fp32 roundings of z that libm and ocml may place differently.
Histograms: 1e-12 * B as for ti_obs_hist.  With TI_ZMAT_PARITY_OUT set, the worst observed ratio to each bound is appended there
(profiles/zmat_parity.txt)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from conftest import load_golden, pkg
import obs_numpy as on
import zmat_numpy as zn

pytestmark = pytest.mark.gpu

ATOMS = (2, 3, 4, 5, 18, 32)
BATCHES = (1, 63, 64, 65, 257, 4099)          # one; around the 64 molecules of a workgroup; several blocks of either kernel
B_FULL = max(BATCHES)
RATIOS = {}


def note(name, ratio):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(ratio))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


@functools.lru_cache(maxsize=None)
def engine(A):
    """A PaiNN handle for A atoms (the smallest model: the Z-matrix calls need the handle's species size only)"""
    ti = pkg()
    syn, W = ti.synthetic, ti.weights
    src, dst, et = syn.fully_connected_template(A)
    flat = W.flatten_state_dict(syn.painn_state_dict(0, 32, 1, 25, seed=1), W.painn_param_spec(0, 32, 1, 25))
    return ti.engine.PainnEngine(0, 32, 1, A, src, dst, et, np.arange(A) % 25, flat, temp_length=100.0)      # 25 atom types


@functools.lru_cache(maxsize=None)
def case(A):
    """(ZMatrix, z_in [B,A-1,3] f32, x [B,A,3] f32, references) of a random tree over relabelled atoms; computed once.  Every 7th
    molecule has one entry pushed out of the valid range (the placement does not mind: it does not clamp)."""
    rs = np.random.RandomState(100 + A)
    label = rs.permutation(A)
    bonds = np.array([[label[i], label[rs.randint(0, i)]] for i in range(1, A)])
    order, ref = zn.from_bonds(bonds, A, int(label[0]))
    zm = pkg().zmatrix.ZMatrix(order, ref)
    z = np.zeros((B_FULL, A - 1, 3))
    z[:, :, 0] = rs.uniform(0.9, 1.6, (B_FULL, A - 1))
    z[:, 1:, 1] = rs.uniform(1.2, 2.6, (B_FULL, max(A - 2, 0)))
    z[:, 2:, 2] = rs.uniform(-3.1, 3.1, (B_FULL, max(A - 3, 0)))
    z = z.astype(np.float32)
    z[3::7, 0, 0] *= -1.0
    if A >= 4:
        z[5::7, -1, 2] = -zn.PI32
    x64, logdet, absum, _ = zn.deconstruct(z, order, ref)
    x = x64.astype(np.float32)
    return dict(zm=zm, z_in=z, x=x, x64=x64, logdet=logdet, absum=absum, valid=zn.valid_mask(z), z64=zn.construct(x, order, ref))


def cv_equivalent(eng, zm, x):
    """z [B, A-1, 3] assembled from ti_obs_cv with the equivalent descriptors; structural zeros stay 0"""
    desc = zm.descriptors()
    live = [i for i, d in enumerate(desc) if d is not None]
    cv = eng.collective_variables(x, [desc[i] for i in live])
    out = np.zeros((x.shape[0], 3 * (zm.A - 1)), np.float32)
    out[:, live] = cv
    return out.reshape(x.shape[0], zm.A - 1, 3)


# ------------------------------------------------------------------------------------------------------------ x -> z
@pytest.mark.parametrize("A", ATOMS)
def test_zmat_is_ti_obs_cv_bit_for_bit_and_within_the_cv_bound(A):
    c, eng = case(A), engine(A)
    zm, x = c["zm"], c["x"]
    for B in BATCHES:
        z = eng.zmatrix(x[:B], zm)
        assert z.shape == (B, A - 1, 3) and z.dtype == np.float32
        np.testing.assert_array_equal(bits(z), bits(cv_equivalent(eng, zm, x[:B])), err_msg=f"A={A} B={B}")
        assert (bits(z[:, 0, 1:]) == 0).all() and (A < 3 or (bits(z[:, 1, 2]) == 0).all())          # structural zeros: +0 exactly
        ref = c["z64"][:B]
        r = np.abs(z - ref) / (1e-6 * (1 + np.abs(ref)))
        note("zmat / cv bound", r.max())
        assert r.max() <= 1.0, (A, B, r.max())
    np.testing.assert_array_equal(bits(pkg().observables.zmatrix(eng, x[:5], (zm.order, zm.ref))), bits(eng.zmatrix(x[:5], zm)))


def fixture_cases():
    g = load_golden("zmat_reference")
    return [{k[len(f"c{i}_"):]: v for k, v in g.items() if k.startswith(f"c{i}_")} for i in range(len(g["cases"]))]


def test_both_calls_against_the_reference_fixture():
    ti = pkg()
    for c in fixture_cases():
        A = c["x"].shape[1]
        eng, zm = engine(A), ti.zmatrix.ZMatrix(c["order"], c["ref"])
        e_z, e_x, e_ld = c["e_ref"]
        z = eng.zmatrix(c["x"], zm)
        r = np.abs(z - c["z_ref"]) / (e_z + 1e-6 * (1 + np.abs(c["z_ref"])))
        note("zmat / fixture", r.max())
        assert r.max() <= 1.0, (A, r.max())
        x, ld = eng.zmatrix_xyz(c["z_in"], zm, logdet=True)
        scale = np.abs(c["x_ref"]).max(axis=(1, 2), keepdims=True)
        r = np.abs(x - c["x_ref"]) / (e_x + 1e-6 * (1 + scale))
        note("xyz / fixture", r.max())
        assert r.max() <= 1.0, (A, r.max())
        _, _, absum, _ = zn.deconstruct(c["z_in"], c["order"], c["ref"])
        for name in ("logdet_ref", "logdet2_ref"):
            r = np.abs(ld - c[name]) / (e_ld + 8 * 3 * A * 2.0 ** -53 * (1 + absum))
            note("logdet / fixture", r.max())
            assert r.max() <= 1.0, (A, name, r.max())
    g = load_golden("zmat_reference")
    zv = g["valid_z"]
    _, valid = engine(4).zmatrix_xyz(zv, ti.zmatrix.ZMatrix(None, [[0, 0, 0], [0, 0, 0], [1, 0, 0], [2, 1, 0]]), valid=True)
    np.testing.assert_array_equal(valid, g["valid_mask"])


# ------------------------------------------------------------------------------------------------------------ z -> x
@pytest.mark.parametrize("A", ATOMS)
def test_zmat_xyz_against_the_restatement(A):
    c, eng = case(A), engine(A)
    zm, z = c["zm"], c["z_in"]
    for B in BATCHES:
        x, ld, valid = eng.zmatrix_xyz(z[:B], zm, logdet=True, valid=True)
        assert x.shape == (B, A, 3) and x.dtype == np.float32 and ld.dtype == np.float64 and valid.dtype == np.uint8
        ref = c["x64"][:B]
        r = np.abs(x - ref) / (1e-6 * (1 + np.abs(ref).max(axis=(1, 2), keepdims=True)))
        note("xyz / coordinate bound", r.max())
        assert r.max() <= 1.0, (A, B, r.max())
        r = np.abs(ld - c["logdet"][:B]) / (8 * 3 * A * 2.0 ** -53 * (1 + c["absum"][:B]))
        note("logdet / bound", r.max())
        assert r.max() <= 1.0, (A, B, r.max())
        np.testing.assert_array_equal(valid, c["valid"][:B])
        if A == 2:
            assert (ld == 0).all()
    assert 0 < c["valid"].sum() < B_FULL
    # the outputs that were not asked for change nothing
    x_only = eng.zmatrix_xyz(z[:65], zm)
    np.testing.assert_array_equal(bits(x_only), bits(eng.zmatrix_xyz(z[:65], zm, logdet=True)[0]))


@pytest.mark.parametrize("A", (4, 18, 32))
def test_round_trip_rmsd(A):
    c, eng = case(A), engine(A)
    zm = c["zm"]
    rs = np.random.RandomState(A)
    n = 6
    q, _ = np.linalg.qr(rs.standard_normal((3, 3)))
    q *= np.sign(np.linalg.det(q))
    ok = np.flatnonzero(c["valid"])[:n]
    x = (c["x64"][ok] @ q.T + rs.standard_normal(3)).astype(np.float32)                  # out of the canonical frame
    x2 = eng.zmatrix_xyz(eng.zmatrix(x, zm), zm)
    z32 = zn.construct(x, zm.order, zm.ref).astype(np.float32)
    x2_ref, _, _, _ = zn.deconstruct(z32, zm.order, zm.ref)
    for b in range(n):
        got = float(eng.collective_variables(x2[b:b + 1], [("rmsd",)], ref=x[b])[0, 0])
        want = float(on.kabsch_rmsd(x2_ref[b:b + 1], x[b])[0])
        bound = 2.0 * want + 1e-6 * float(on.rmsd_scale(x2[b:b + 1], x[b])[0])
        note("round trip rmsd / bound", got / bound)
        assert got <= bound, (A, b, got, want)


# ------------------------------------------------------------------------------------------------------------ invariances
@pytest.mark.parametrize("A", (3, 18))
def test_batch_order_and_memory_space_do_not_enter(A):
    import torch
    c, eng = case(A), engine(A)
    zm, B = c["zm"], 257
    x, z = c["x"][:B], c["z_in"][:B]
    perm = np.random.RandomState(1).permutation(B)
    zo = eng.zmatrix(x, zm)
    xo, ld, valid = eng.zmatrix_xyz(z, zm, logdet=True, valid=True)
    np.testing.assert_array_equal(bits(eng.zmatrix(np.ascontiguousarray(x[perm]), zm)), bits(zo[perm]))
    xp, lp, vp = eng.zmatrix_xyz(np.ascontiguousarray(z[perm]), zm, logdet=True, valid=True)
    np.testing.assert_array_equal(bits(xp), bits(xo[perm])); np.testing.assert_array_equal(bits(lp), bits(ld[perm]))
    np.testing.assert_array_equal(vp, valid[perm])
    np.testing.assert_array_equal(bits(eng.zmatrix(x[40:41], zm)), bits(zo[40:41]))          # alone
    np.testing.assert_array_equal(bits(eng.zmatrix(x, zm)), bits(zo))                          # again
    zd = eng.zmatrix(torch.from_numpy(x).cuda(), zm)
    assert zd.is_cuda
    np.testing.assert_array_equal(bits(zd.cpu().numpy()), bits(zo))
    xd, ldd, vd = eng.zmatrix_xyz(torch.from_numpy(z).cuda(), zm, logdet=True, valid=True)
    assert xd.is_cuda and ldd.dtype == torch.float64 and vd.dtype == torch.uint8
    np.testing.assert_array_equal(bits(xd.cpu().numpy()), bits(xo)); np.testing.assert_array_equal(bits(ldd.cpu().numpy()), bits(ld))
    np.testing.assert_array_equal(vd.cpu().numpy(), valid)


def test_degenerate_molecules_poison_only_themselves():
    A = 5
    c, eng = case(A), engine(A)
    zm, B = c["zm"], 70
    x, z = c["x"][:B].copy(), c["z_in"][:B].copy()
    clean_z = eng.zmatrix(x, zm)
    clean_x, clean_ld, clean_v = eng.zmatrix_xyz(z, zm, logdet=True, valid=True)
    x[5, int(zm.order[0]), 1] = np.nan                        # the root: every row of molecule 5 that reaches it
    x[9, int(zm.order[2])] = x[9, int(zm.order[1])]           # coinciding atoms: a zero-length reference
    zb = eng.zmatrix(x, zm)
    others = np.setdiff1d(np.arange(B), [5, 9])
    np.testing.assert_array_equal(bits(zb[others]), bits(clean_z[others]))
    assert np.isnan(zb[5]).any() and (bits(zb[5, 0, 1:]) == 0).all()
    z[5, 1, 0] = np.nan                                       # a NaN distance
    z[9, 1, 1] = 0.0                                          # sorted atoms 0, 1, 2 on a line: the frame of atom 3 is 0 / 0
    z[12, 3, 0] = 0.0                                         # d = 0: log 0
    xb, ldb, vb = eng.zmatrix_xyz(z, zm, logdet=True, valid=True)
    others = np.setdiff1d(np.arange(B), [5, 9, 12])
    np.testing.assert_array_equal(bits(xb[others]), bits(clean_x[others])); np.testing.assert_array_equal(bits(ldb[others]), bits(clean_ld[others]))
    np.testing.assert_array_equal(vb[others], clean_v[others])
    assert np.isnan(xb[5]).any() and np.isnan(ldb[5]) and vb[5] == 0
    assert np.isnan(xb[9, int(zm.order[3])]).all() and vb[9] == 1          # a = 0 is inside the valid range
    assert ldb[12] == -np.inf and vb[12] == 0 and np.isfinite(xb[12]).all()


# ------------------------------------------------------------------------------------------------------------ refusals
def raw_zmat(h, order, ref, x, A):
    ti = pkg()
    out = np.full((x.shape[0], A - 1, 3), 7.0, np.float32)
    ip = lambda a: None if a is None else ti._lib.iptr(a)
    rc = ti._lib.lib().ti_obs_zmat(h, ip(order), ip(ref), C.c_void_p(x.ctypes.data), x.shape[0], C.c_void_p(out.ctypes.data), 0)
    return rc, out


def test_refusals_write_nothing():
    ti = pkg()
    E, U = ti._lib.TI_E_ARG, ti._lib.TI_E_UNSUPPORTED
    A = 4
    eng, c = engine(A), case(A)
    x = c["x"][:3]
    order, ref = np.arange(A, dtype=np.int32), np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [2, 1, 0]], np.int32)
    rc, out = raw_zmat(eng.h, None, ref, x, A)
    assert rc == 0 and (out != 7.0).all()
    bad = [(np.array([0, 1, 2, 2], np.int32), ref, "permutation"), (np.array([0, 1, 2, 4], np.int32), ref, "permutation"),
           (order, np.array([[0, 0, 0], [1, 0, 0], [1, 0, 0], [2, 1, 0]], np.int32), "earlier sorted atom"),
           (order, np.array([[0, 0, 0], [0, 0, 0], [1, 1, 0], [2, 1, 0]], np.int32), "repeats"),
           (order, np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [2, 1, -1]], np.int32), "earlier sorted atom"), (order, None, "ref is NULL")]
    for o, r, msg in bad:
        rc, out = raw_zmat(eng.h, o, r, x, A)
        assert rc == E and msg in ti._lib.last_error() and (out == 7.0).all(), (msg, ti._lib.last_error())
    xyz = np.full((3, A, 3), 7.0, np.float32)
    rc = ti._lib.lib().ti_obs_zmat_xyz(eng.h, None, ti._lib.iptr(bad[2][1]), C.c_void_p(c["z_in"][:3].ctypes.data), 3, C.c_void_p(xyz.ctypes.data), None, None, 0)
    assert rc == E and (xyz == 7.0).all()
    # an adw handle
    W, syn = ti.weights, ti.synthetic
    adw = ti.engine.AdwEngine(32, 2, W.flatten_state_dict(syn.adw_state_dict(32, 2), W.adw_param_spec(32, 2), dtype=np.float64))
    rc, out = raw_zmat(adw.h, None, ref, x, A)
    assert rc == E and "not a painn handle" in ti._lib.last_error() and (out == 7.0).all()
    # mixed species in force: one topology is one species
    eng.set_molecules(np.array([4, 3, 4], np.int32))
    try:
        rc, out = raw_zmat(eng.h, None, ref, x, A)
        assert rc == U and "one species" in ti._lib.last_error() and (out == 7.0).all()
        with pytest.raises(ti._lib.TiError):
            eng.zmatrix_xyz(c["z_in"][:3], c["zm"])
    finally:
        eng.set_molecules(None)
    rc, out = raw_zmat(eng.h, None, ref, x, A)
    assert rc == 0
    # B = 0 is fine and touches nothing
    assert ti._lib.lib().ti_obs_zmat(eng.h, None, ti._lib.iptr(ref), None, 0, None, 0) == 0


# ------------------------------------------------------------------------------------------------------------ ti_obs_hist_cols
H_BATCHES = (1, 255, 256, 257, 2049, 5000)      # around one block of 256; all 8 blocks with more than one trip
H_BINS = (1, 64, 256)


@functools.lru_cache(maxsize=None)
def hist_inputs(K):
    rs = np.random.RandomState(K)
    B = max(H_BATCHES)
    v = (rs.standard_normal((B, K)) * 0.8).astype(np.float32)
    v[rs.randint(0, B, 40), rs.randint(0, K, 40)] = np.nan
    v[rs.randint(0, B, 10), rs.randint(0, K, 10)] = np.inf
    logw = (rs.standard_normal(B) * 2.0).astype(np.float32)
    keep = (rs.uniform(size=B) < 0.7).astype(np.uint8)
    keep[0] = 1
    lo, hi = -1.0 - 0.01 * np.arange(K), 1.0 + 0.02 * np.arange(K)
    v[7 % B, 0] = np.float32(hi[0])                                # hi itself: the upper tail
    return v, logw, keep, lo, hi


@pytest.mark.parametrize("K", (1, 3, 48, 93))
def test_hist_cols_is_ti_obs_hist_per_column_and_masks_the_weights(K):
    eng = engine(4)
    v_all, logw_all, keep_all, lo, hi = hist_inputs(K)
    for i, B in enumerate(H_BATCHES):
        for bins in (H_BINS if B in (257, 5000) else (H_BINS[i % 3],)):
            v, logw, keep = np.ascontiguousarray(v_all[:B]), logw_all[:B], keep_all[:B]
            for lw in (logw, None):
                hist, tails = eng.hist_cols(v, lw, None, bins, lo, hi)
                assert hist.shape == (K, bins) and tails.shape == (K, 3)
                for c in (range(K) if lw is not None or K <= 3 else (0, K - 1)):
                    h1, t1 = eng.weighted_histogram(v[:, c], lw, bins, (lo[c], hi[c]))
                    np.testing.assert_array_equal(bits(hist[c]), bits(h1), err_msg=f"K={K} B={B} bins={bins} column {c}")
                    np.testing.assert_array_equal(bits(tails[c]), bits(t1))
                assert np.abs(hist.sum(axis=1) + tails.sum(axis=1) - 1.0).max() <= 1e-12 * B
                # the mask: the oracle on the compacted arrays
                hist, tails = eng.hist_cols(v, lw, keep, bins, lo, hi)
                sel = keep != 0
                for c in range(K):
                    h0, t0 = on.weighted_histogram(v[sel, c], None if lw is None else lw[sel], bins, lo[c], hi[c])
                    r = max(np.abs(hist[c] - h0).max(), np.abs(tails[c] - t0).max()) / (1e-12 * B)
                    note("hist_cols keep / bound", r)
                    assert r <= 1.0, (K, B, bins, c, r)
                assert np.abs(hist.sum(axis=1) + tails.sum(axis=1) - 1.0).max() <= 1e-12 * B
    if K == 1:
        assert eng.hist_cols(v_all[:256], None, None, 4, lo, hi)[1][0, 1] > 0          # the value equal to hi is in the upper tail


def test_hist_cols_device_memory_and_refusals():
    import torch
    ti = pkg()
    eng = engine(4)
    K, B, bins = 3, 2049, 64
    v, logw, keep, lo, hi = hist_inputs(K)
    v, logw, keep = np.ascontiguousarray(v[:B]), logw[:B].copy(), keep[:B].copy()
    host = eng.hist_cols(v, logw, keep, bins, lo, hi)
    dev = eng.hist_cols(torch.from_numpy(v).cuda(), torch.from_numpy(logw).cuda(), torch.from_numpy(keep).cuda(), bins, lo, hi)
    np.testing.assert_array_equal(bits(dev[0]), bits(host[0])); np.testing.assert_array_equal(bits(dev[1]), bits(host[1]))
    np.testing.assert_array_equal(bits(eng.hist_cols(v, logw, keep, bins, lo, hi)[0]), bits(host[0]))            # again
    # the service engine (an adw handle) takes the call as well: through observables.zmatrix_marginals
    z = np.ascontiguousarray(case(5)["z_in"][:300])
    m = ti.observables.zmatrix_marginals(z, logw[:300], keep[:300], bins=16, length_range=(0.5, 2.0))
    assert m.hist.shape == (9, 16) and m.tails.shape == (9, 3) and m.ranges.shape == (9, 2)
    cols = ti.zmatrix.marginal_columns(5)
    sel = keep[:300] != 0
    for j, cidx in enumerate(cols):
        h0, t0 = on.weighted_histogram(z.reshape(300, -1)[sel, cidx], logw[:300][sel], 16, *m.ranges[j])
        assert np.abs(m.hist[j] - h0).max() <= 1e-12 * 300 and np.abs(m.tails[j] - t0).max() <= 1e-12 * 300
    np.testing.assert_array_equal(m.ranges[[0, 4, 7]], [[0.5, 2.0], [0.0, np.pi], [-np.pi, np.pi]])
    # a non-finite logw: refused by index when kept, invisible when not
    unkept, kept = int(np.flatnonzero(keep == 0)[3]), int(np.flatnonzero(keep)[5])
    logw[unkept] = np.nan
    np.testing.assert_array_equal(bits(eng.hist_cols(v, logw, keep, bins, lo, hi)[0]), bits(host[0]))
    logw[kept] = np.inf
    with pytest.raises(ti._lib.TiError, match=f"non-finite logw at index {kept}$") as ei:
        eng.hist_cols(v, logw, keep, bins, lo, hi)
    assert ei.value.code == ti._lib.TI_E_NAN
    with pytest.raises(ti._lib.TiError, match=f"non-finite logw at index {min(kept, unkept)}$"):
        eng.hist_cols(v, logw, None, bins, lo, hi)
    with pytest.raises(ti._lib.TiError, match="keeps no entry") as ei:
        eng.hist_cols(v, None, np.zeros(B, np.uint8), bins, lo, hi)
    assert ei.value.code == ti._lib.TI_E_ARG
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    out_h, out_t = np.zeros((K, bins)), np.zeros((K, 3))
    call = lambda k, nb, l, h: ti._lib.lib().ti_obs_hist_cols(eng.h, C.c_void_p(v.ctypes.data), k, None, None, B, nb, dp(l), dp(h), dp(out_h), dp(out_t), 0)
    assert call(K, bins, lo, hi) == 0
    for args in ((0, bins, lo, hi), (129, bins, lo, hi), (K, 0, lo, hi), (K, 257, lo, hi), (K, bins, hi, lo), (K, bins, lo, np.full(K, np.inf))):
        assert call(*args) == ti._lib.TI_E_ARG, args[:2]


def test_record_parity():
    """Last in the file: prints the worst ratio to every bound seen above and, with TI_ZMAT_PARITY_OUT set, appends them there"""
    lines = [f"{name:28s} worst observed / bound = {r:.3e}" for name, r in sorted(RATIOS.items())]
    print("\n".join(lines))
    out = os.environ.get("TI_ZMAT_PARITY_OUT")
    if out and lines:
        with open(out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
