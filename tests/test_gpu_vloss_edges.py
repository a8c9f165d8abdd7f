"""Velocity loss beyond one workgroup and one tile (tests/test_gpu_vloss.py holds it to the reference at B <= 32, where blockIdx.x is 0 in
every kernel of csrc/vloss_kernels.hip): batch-wide sums over several tiles and past the 256-tile stride of the combine, adw handles in
d > 1 dimensions, molecule ids with a high counter word, the pad molecules of the packed layouts at every slot, the value edges of
the time range, and the first non-finite row anywhere but row 0.  Every check is against the fp64 restatement (tests/vloss_numpy.py),
the host oracle's normal, or the engine's own drift entry; nothing here is recorded from the reference.

Bit-for-bit checks.  Centring: on vloss_numpy.dyadic_case every product and every column sum is exact in fp64, so the only roundings
are the division of the mean, the subtraction and the cast, each correctly rounded on both sides (tests/test_vloss_host.py proves the
premise in rational arithmetic).  Mean and time profile: fp64 adds in the order include/ti_hip.h states, restated by
vloss_numpy.fixed_order_sum / time_bins_fixed_order, which the host tests hold to a thread-by-thread transcription of the kernels.

Bounds (printed as the worst ratio to the bound, `pytest -s`).  Stage one: 2^-23 S, as in tests/test_gpu_vloss.py, plus under
TI_CENTER_BATCH 2 E_c with E_c = 2^-53 sum over the rows of |raw_c|: a sum of n terms in any order errs by at most (n - 1) 2^-53 sum|v|
and the mean divides it by n; the factor 2 covers the restatement's own sum.  One row lost from 2500 moves the mean by about 4e-4 of a
coordinate, four decades above.  Reduce: 2 n_terms 2^-53 sum|terms|."""
import ctypes as C

import numpy as np
import pytest

import adw_nd_numpy as nd
import vloss_numpy as vn
from conftest import pkg, rel_l2
from test_gpu_vloss import PRECISIONS, U, _reduce_ok, _setup, _small, _vn_kw

pytestmark = pytest.mark.gpu
F32 = np.float32
ALL = ("t", "z", "xt", "b")
GAMMAS = {"brownian": 0.9, "sin2": 1.0, "sig_sum": 4.0}


# ------------------------------------------------------------------------------------------------ helpers
def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def _stage_one(tag, xt, x0, x1, t, z, center, **kw):
    """|xt - xt64| <= 2^-23 S (+ 2 E_c under BATCH); prints and returns the worst ratio"""
    xt64, S, E = vn.interpolate(x0, x1, t, z, center=center, return_abs=True, **kw)
    bound = 2.0 ** -23 * S
    if center == "batch":
        bound = bound + 2 * U * E.reshape((E.shape[0],) + (1,) * (S.ndim - 2) + E.shape[1:])
    err = np.abs(xt.astype(np.float64) - xt64)
    assert xt.shape == xt64.shape and (bound > 0).any()
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"vloss-edges {tag}: stage one, max |xt - xt64| / bound {ratio:.3f}")
    assert (err <= bound).all(), ratio
    return ratio


def _reduce(tag, r, x0, x1, s_kw):
    """loss against vn.loss fed the call's own t, z and b, within 2 n_terms 2^-53 sum|terms|"""
    b = _np(r["b"])
    l, mag, n_terms = vn.loss(x0, x1, _np(r["t"]), _np(r["z"]) if "z" in r else None, b[0], b[1] if b.shape[0] == 2 else None, **s_kw)
    loss = _np(r["loss"])
    assert loss.dtype == np.float64 and loss.shape == l.shape and np.isfinite(loss).all()
    bound = 2 * n_terms * U * mag
    ratio = float((np.abs(loss - l)[bound > 0] / bound[bound > 0]).max())
    print(f"vloss-edges {tag}: reduce, max |loss - vn.loss| / bound {ratio:.3f}")
    assert (np.abs(loss - l) <= bound).all(), ratio
    return ratio


def _ambient(precision="f32"):
    eng, call, interp, s, g, c = _setup("vloss_ambient", "brownian", precision)
    return eng, g, c


def _adw_fixture():
    eng, call, interp, s, g, c = _setup("vloss_adw_h64", "standard")
    return eng, float(g["a"])


def _adw_inputs(B, seed):
    rs = np.random.RandomState(seed)
    return ((1.2 * rs.standard_normal(B)).astype(F32), (0.9 * rs.standard_normal(B)).astype(F32), rs.uniform(0.5, 1.5, B).astype(F32),
            rs.uniform(0.75, 2.0, B).astype(F32))


def _molecules(B, A, seed):
    syn = pkg().synthetic
    return syn.molecule_coords(B, A, seed=seed), syn.molecule_coords(B, A, seed=seed + 1), syn.ambient_cond(B, A)


_CELLS = {}


def _cell(H, d, L, precision="f32"):
    """(engine, state dict) of a cell of adw_nd_numpy.MATRIX"""
    assert (H, d, L) in nd.MATRIX
    key = (H, d, L, precision)
    if key not in _CELLS:
        ti = pkg()
        sd = nd.cell_state_dict(H, L, d)
        flat = ti.weights.flatten_state_dict(sd, ti.weights.adw_param_spec(H, L, d, d), dtype=np.float64)
        _CELLS[key] = (ti.engine.AdwEngine(H, L, flat, precision=precision, dim=d), sd)
    return _CELLS[key]


def _cell_pairs(d, B=300):
    """cell_inputs(d, B) as x0, with x1 a second draw of the same kind"""
    inp = nd.cell_inputs(d, B)
    x1 = (np.random.RandomState(9000 + d).standard_normal((B, d)) * np.linspace(0.3, 3.0, B)[:, None]).astype(F32)
    return inp.x, x1, inp.b0, inp.b1


def _oracle_z(seed, off, draw, B, m):
    from oracle import oracle
    return np.asarray([[oracle.normal(seed, off + b, draw, k) for k in range(m)] for b in range(B)], F32)


# ------------------------------------------------------------------------------------------------ 4a. centring across tiles, bit for bit
@pytest.mark.parametrize("which,B", [("small", 513), ("small", 1250), ("small", 131073), ("ambient", 171)])
def test_centring_across_tiles_bit_for_bit(which, B):
    """One-sided states of dyadic_case: 1026 rows (two tiles, a tail of 2; with A = 2 and with A = 6, m = 18), 2500 rows, and 262 146
    rows = 257 tiles, where the combine takes its stride of 256.  xt is float32(raw - colsum / rows) of numpy for BATCH, float32(raw -
    molecule mean) for MOLECULE, float32(raw) for NONE, by array_equal: a row lost or counted twice at a tile edge moves every entry."""
    eng = _small() if which == "small" else _ambient()[0]
    x0, x1, t = vn.dyadic_case(B, eng.A, seed=B)
    for center in ("batch", "molecule", "none"):
        r = eng.interpolate(x0, x1, kind="one_sided", center=center, t=t)
        ref = vn.interpolate(x0, x1, t, kind="one_sided", center=center)[0].astype(F32)
        assert r["xt"].shape == (1, B, eng.A, 3) and r["xt"].dtype == F32
        assert np.array_equal(r["xt"], ref), (center, int((r["xt"] != ref).sum()))
        assert np.array_equal(r["t"], t)
    assert np.abs(vn.interpolate(x0, x1, t, kind="one_sided", center="none")[0].reshape(-1, 3).mean(axis=0)).max() > 1e-4          # a centre to remove


# ------------------------------------------------------------------------------------------------ 4b. both halves across tiles, by bound
@pytest.mark.parametrize("gamma", sorted(GAMMAS))
def test_both_halves_across_three_ragged_tiles(gamma):
    """Standard loss on the ambient fixture's species, BATCH, B = 417: 2502 rows, three tiles, the last ragged, for each of the two
    column-sum launches (plus at colsum 0..2, minus at 3..5, raw + n)."""
    eng, g, _ = _ambient()
    B, A = 417, eng.A
    x0, x1, cond = _molecules(B, A, 41)
    kw = dict(gamma=gamma, a=GAMMAS[gamma], center="batch", seed=12, draw=1)
    s_kw = dict(gamma_kind=gamma, a=GAMMAS[gamma])
    ri = eng.interpolate(x0, x1, **kw)
    _stage_one(f"ambient B 417 {gamma} interpolate", ri["xt"], x0, x1, ri["t"], ri["z"], "batch", **s_kw)
    r = eng.velocity_loss(x0, x1, cond, returns=ALL, **kw)
    for k in ("t", "z", "xt"):
        assert np.array_equal(r[k], ri[k]), k
    _reduce(f"ambient B 417 {gamma}", r, x0, x1, s_kw)
    assert r["rows"] == B * A
    for half in (0, 1):
        e = rel_l2(r["b"][half], eng.drift(r["xt"][half], r["t"], cond))
        print(f"vloss-edges ambient B 417 {gamma}: rel_l2(b[{half}], drift(xt[{half}])) {e:.2e}")
        assert e < 1e-6


# ------------------------------------------------------------------------------------------------ 4c. mean and time profile in the fixed order
def _mean_and_drift(tag, eng, r, x0, conds):
    assert r["loss"].shape == (x0.shape[0],)
    assert r["mean"] == vn.fixed_order_sum(r["loss"]) / r["rows"], (tag, r["mean"], vn.fixed_order_sum(r["loss"]) / r["rows"])
    for half in range(r["b"].shape[0]):
        assert np.array_equal(r["b"][half], eng.drift(r["xt"][half], r["t"], *conds)), (tag, half)


def _tbins_exact(r, n):
    B = r["loss"].shape[0]
    assert r["tbins"].shape == (n, 2) and r["tbins"][:, 1].sum() == B
    assert np.array_equal(r["tbins"][:, 1], vn.time_bins(r["loss"], r["t"], n)[:, 1])
    assert np.array_equal(r["tbins"], vn.time_bins_fixed_order(r["loss"], r["t"], n))


ADW_B = [257, 1024, 1025, 2500, 263000]
_ADW_CALLS = {}


def _adw_call(B, n=0):
    """(inputs, result) of the adw fixture engine's loss call over B rows with n time bins, made once"""
    if (B, n) not in _ADW_CALLS:
        eng, a = _adw_fixture()
        inp = _adw_inputs(B, B)
        _ADW_CALLS[B, n] = (inp, eng.velocity_loss(*inp, a=a, seed=5, draw=1, tbins=n, returns=ALL))
    return _ADW_CALLS[B, n]


@pytest.mark.parametrize("B", ADW_B)
def test_mean_and_time_profile_in_the_fixed_order(B):
    """adw fixture engine (H 64, d 1), drawn t and z.  B = 257: two blocks of every per-row kernel; 1024 / 1025: one tile exactly, and
    one row into the second; 2500: three tiles, ragged; 263 000: 257 tiles with a tail of 856, the combine's second round.  The mean
    is fixed_order_sum(loss) / B and the profile time_bins_fixed_order(loss, t), exactly; each half of b is the drift entry's bits."""
    eng, a = _adw_fixture()
    for n in {2500: (1, 7, 1024), 263000: (7,)}.get(B, (0,)):
        (x0, x1, b0, b1), r = _adw_call(B, n)
        assert np.array_equal(r["t"], vn.draw_t("uniform", 5, 0, 1, B)) and r["rows"] == B
        if n:
            _tbins_exact(r, n)
    _mean_and_drift(f"adw d 1 B {B}", eng, r, x0, (b0, b1))


@pytest.mark.parametrize("B", ADW_B)
def test_adw_loss_beyond_one_block_within_the_reduce_bound(B):
    """vloss_reduce_kernel past block 0: the reduce bound of tests/test_gpu_vloss.py, 2 n_terms 2^-53 sum|terms|, on the same calls.
    With m = 1 a row has four terms, and among a thousand rows some have d = x1 - x0 and gamma' z cancel to a few parts in a thousand;
    there the rounding of gamma' z is hundreds of times the rounding of the term d + gamma' z that this bound counts.  A kernel that
    fused d + gamma' z into one fma was up to 3.6 times over the bound on such rows (1.81, 1.39, 3.56, 3.09 at B = 1024, 1025, 2500,
    263 000); the kernel rounds every operation on its own (contraction off), as the restatement does, and the ratio is 0."""
    (x0, x1, b0, b1), r = _adw_call(B, {2500: 7, 263000: 7}.get(B, 0))
    _reduce(f"adw d 1 B {B}", r, x0, x1, dict(a=_adw_fixture()[1]))


def test_host_and_device_memory_give_the_same_bits():
    import torch
    eng, a = _adw_fixture()
    B = 2500
    x0, x1, b0, b1 = _adw_inputs(B, B)
    kw = dict(a=a, seed=5, draw=1, tbins=7, returns=ALL)
    host = eng.velocity_loss(x0, x1, b0, b1, **kw)
    dev = eng.velocity_loss(*(torch.from_numpy(v).cuda() for v in (x0, x1, b0, b1)), **kw)
    assert dev["loss"].is_cuda and dev["t"].is_cuda and dev["mean"] == host["mean"]
    for k in ("loss", "tbins", "t", "z", "xt", "b"):
        assert np.array_equal(_np(dev[k]), host[k]), k


def test_mean_of_molecules_in_the_fixed_order():
    """The same three checks on molecules: _small() (A 2), standard, MOLECULE, B = 700 -- 1400 rows, and the divisor is rows = B A while
    the sum runs over the B losses.  With the layout pinned each half of b is the drift entry's bits: molecule b of either half lies
    at slot b mod G of its row group, as it does in a drift call over the half alone (include/ti_hip.h, Drift)."""
    eng = _small()
    B = 700
    x0, x1, cond = _molecules(B, 2, 51)
    eng.set_template("latency")
    try:
        r = eng.velocity_loss(x0, x1, cond, gamma="sin2", center="molecule", seed=6, tbins=7, returns=ALL)
        assert r["rows"] == 2 * B
        _tbins_exact(r, 7)
        _mean_and_drift("small B 700 molecule", eng, r, x0, (cond,))
    finally:
        eng.set_template("auto")
    _reduce("small B 700 molecule", r, x0, x1, dict(gamma_kind="sin2"))
    _stage_one("small B 700 molecule", r["xt"], x0, x1, r["t"], r["z"], "molecule", gamma_kind="sin2")


# ------------------------------------------------------------------------------------------------ 4d. adw in d dimensions
CELLS = [(64, 5, 3), (32, 16, 2), (256, 2, 1)]          # a counter-word crossing at k = 4; four words; Kpad exact
SEED_ND, OFF_ND, DRAW_ND = 0x123456789A, 11, 3


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("H,d,L", CELLS)
def test_adw_in_d_dimensions(H, d, L, precision):
    """m = d: the noise of coordinate k is component k of the draw (word k >> 2 of the counter), the states are [B, d] rows, and the
    drift is the d-dimensional kernel on 2B rows.  B = 300: two blocks of the per-row kernels, up to 19 of the per-entry ones."""
    eng, sd = _cell(H, d, L, precision)
    x0, x1, b0, b1 = _cell_pairs(d)
    B = x0.shape[0]
    tag = f"adw H {H} d {d} L {L} {precision}"
    kw = dict(a=0.9, seed=SEED_ND, traj_offset=OFF_ND, draw=DRAW_ND)
    r = eng.velocity_loss(x0, x1, b0, b1, returns=ALL, **kw)
    assert r["z"].shape == (B, d) and r["xt"].shape == (2, B, d) and r["b"].shape == (2, B, d)
    assert np.array_equal(r["z"], _oracle_z(SEED_ND, OFF_ND, DRAW_ND, B, d))
    assert np.array_equal(r["t"], vn.draw_t("uniform", SEED_ND, OFF_ND, DRAW_ND, B))
    _stage_one(tag, r["xt"], x0, x1, r["t"], r["z"], "none", a=0.9)
    for half in (0, 1):
        assert np.array_equal(r["b"][half], eng.drift(r["xt"][half], r["t"], b0, b1)), half
        e = rel_l2(r["b"][half], nd.drift(sd, r["xt"][half], r["t"], b0, b1))
        print(f"vloss-edges {tag}: rel_l2(b[{half}], fp64 drift) {e:.2e}")
        assert e <= 1e-5
    _reduce(tag, r, x0, x1, dict(a=0.9))
    assert r["rows"] == B and r["mean"] == vn.fixed_order_sum(r["loss"]) / B
    ri = eng.interpolate(x0, x1, **kw)
    for k in ("t", "z", "xt"):
        assert np.array_equal(ri[k], r[k]), k
    given = eng.velocity_loss(x0, x1, b0, b1, a=0.9, t=r["t"], z=r["z"], returns=ALL)
    assert given["mean"] == r["mean"]
    for k in ("loss",) + ALL:
        assert np.array_equal(given[k], r[k]), k
    # one-sided: no noise, one half
    tag += " one_sided"
    o = eng.velocity_loss(x0, x1, b0, b1, kind="one_sided", returns=ALL, **{**kw, "a": 1.0})
    assert "z" not in o and o["xt"].shape == (1, B, d) and np.array_equal(o["t"], r["t"])
    _stage_one(tag, o["xt"], x0, x1, o["t"], None, "none", kind="one_sided")
    assert np.array_equal(o["b"][0], eng.drift(o["xt"][0], o["t"], b0, b1))
    assert rel_l2(o["b"][0], nd.drift(sd, o["xt"][0], o["t"], b0, b1)) <= 1e-5
    _reduce(tag, o, x0, x1, dict(kind="one_sided"))
    assert o["mean"] == vn.fixed_order_sum(o["loss"]) / B
    assert np.array_equal(eng.interpolate(x0, x1, kind="one_sided", **kw)["xt"], o["xt"])


# ------------------------------------------------------------------------------------------------ 4e. 64-bit ids
SEED64, DRAW64 = 0xFEDCBA9876543210, 2000000011
OFFSETS64 = [2 ** 32 - 3, 2 ** 40 + 5]          # the low word wraps inside the call; the high word is 256
PARTS = [(slice(0, 1), 0), (slice(1, 3), 1), (slice(3, 6), 3)]


@pytest.mark.parametrize("off", OFFSETS64)
def test_ids_with_a_high_counter_word_draw_what_the_oracle_draws(off):
    """vloss_draw_t_kernel and vl_normal build their counters separately: both against their definition with traj_offset + b past 2^32,
    a seed with both key words set and a draw near 2^31."""
    eng, g, _ = _ambient()
    x0, x1, _ = _molecules(6, eng.A, 31)
    r = eng.interpolate(x0, x1, gamma="brownian", a=0.9, seed=SEED64, traj_offset=off, draw=DRAW64)
    assert np.array_equal(r["z"].reshape(6, -1), _oracle_z(SEED64, off, DRAW64, 6, 3 * eng.A))
    assert np.array_equal(r["t"], vn.draw_t("uniform", SEED64, off, DRAW64, 6))
    ea, a = _adw_fixture()
    xa0, xa1, _, _ = _adw_inputs(32, 3)
    ra = ea.interpolate(xa0, xa1, a=a, seed=SEED64, traj_offset=off, draw=DRAW64)
    assert np.array_equal(ra["z"], _oracle_z(SEED64, off, DRAW64, 32, 1)[:, 0])
    assert np.array_equal(ra["t"], vn.draw_t("uniform", SEED64, off, DRAW64, 32))
    if off >> 32:                                                                 # the high word is in the draw
        assert not np.array_equal(ra["t"], vn.draw_t("uniform", SEED64, off & 0xFFFFFFFF, DRAW64, 32))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("off", OFFSETS64)
def test_split_with_64_bit_ids_bit_for_bit(off, precision):
    """Six in one call against calls of 1, 2 and 3 with traj_offset + 0, + 1, + 3: loss, t and z bit for bit, on the ambient fixture's
    species with the layout pinned as tests/test_gpu_vloss.py pins it (the slot (traj_offset + b) mod G is taken of the 64-bit id) and on adw."""
    eng, g, _ = _ambient(precision)
    x0, x1, cond = _molecules(6, eng.A, 31)
    run = lambda sl, o: eng.velocity_loss(x0[sl], x1[sl], cond[sl], gamma="brownian", a=0.9, center="none", seed=SEED64, draw=DRAW64,
                                          traj_offset=off + o, returns=("t", "z"))
    eng.set_template("latency")
    try:
        whole, split = run(slice(0, 6), 0), [run(sl, o) for sl, o in PARTS]
    finally:
        eng.set_template("auto")
    for k in ("loss", "t", "z"):
        assert np.array_equal(whole[k], np.concatenate([p[k] for p in split])), k
    ea = _setup("vloss_adw_h64", "standard", precision)[0]
    xa0, xa1, b0, b1 = _adw_inputs(6, 3)
    run = lambda sl, o: ea.velocity_loss(xa0[sl], xa1[sl], b0[sl], b1[sl], a=0.9, seed=SEED64, draw=DRAW64, traj_offset=off + o, returns=("t", "z"))
    whole, split = run(slice(0, 6), 0), [run(sl, o) for sl, o in PARTS]
    for k in ("loss", "t", "z"):
        assert np.array_equal(whole[k], np.concatenate([p[k] for p in split])), k


# ------------------------------------------------------------------------------------------------ 4f. slots and pad molecules
@pytest.mark.parametrize("kind", ["standard", "one_sided"])
def test_every_window_of_twelve_equals_its_slice(kind):
    """Ambient fixture's species, layout pinned, NONE: 12 molecules with global ids 0..11 in one call, then every window [offset,
    offset + B) with offset 0..5 and B in {1, 2, 3, 5, 7} as a call of its own with traj_offset = offset, so that `pad` takes every
    slot and `pad2` (standard only) every remainder.  A pad molecule that leaks into a result, or a half read from the wrong place,
    changes loss bits."""
    eng, g, _ = _ambient()
    A = eng.A
    x0, x1, cond = _molecules(12, A, 61)
    kw = dict(kind=kind, gamma="sin2", center="none", seed=21, draw=4, returns=ALL)
    s_kw = dict(kind=kind, gamma_kind="sin2")
    worst, worst_b = 0.0, 0.0
    eng.set_template("latency")
    try:
        ref = eng.velocity_loss(x0, x1, cond, traj_offset=0, **kw)
        for off in range(6):
            for B in (1, 2, 3, 5, 7):
                assert off + B <= 12
                sl = slice(off, off + B)
                r = eng.velocity_loss(x0[sl], x1[sl], cond[sl], traj_offset=off, **kw)
                for k in ("loss", "t") + (("z",) if kind == "standard" else ()):
                    assert np.array_equal(r[k], ref[k][sl]), (off, B, k)
                xt64, S = vn.interpolate(x0[sl], x1[sl], r["t"], r.get("z"), center="none", **s_kw)
                err = np.abs(r["xt"] - xt64)
                assert (err <= 2.0 ** -23 * S).all(), (off, B)
                worst = max(worst, float((err / (2.0 ** -23 * S)).max()))
                for half in range(r["xt"].shape[0]):
                    e = rel_l2(r["b"][half], eng.drift(r["xt"][half], r["t"], cond[sl]))
                    worst_b = max(worst_b, e)
                    assert e < 1e-6, (off, B, half, e)
    finally:
        eng.set_template("auto")
    print(f"vloss-edges windows of 12, {kind}: stage one, max |xt - xt64| / bound {worst:.3f}; max rel_l2(b[half], drift(xt[half])) {worst_b:.2e}")


# ------------------------------------------------------------------------------------------------ 4g. value edges
def test_one_sided_at_the_ends_returns_the_end_states():
    """t x1 + (1 - t) x0 at t = 0 is x0 and at t = 1 is x1, to the bit (NONE)."""
    eng, g, _ = _ambient()
    x0, x1, _ = _molecules(6, eng.A, 31)
    ea, _ = _cell(64, 5, 3)
    xa0, xa1, _, _ = _cell_pairs(5)
    for e, a0, a1 in ((eng, x0, x1), (ea, xa0, xa1)):
        kw = dict(kind="one_sided") if e is ea else dict(kind="one_sided", center="none")
        B = a0.shape[0]
        assert np.array_equal(e.interpolate(a0, a1, t=np.zeros(B, F32), **kw)["xt"][0], a0)
        assert np.array_equal(e.interpolate(a0, a1, t=np.ones(B, F32), **kw)["xt"][0], a1)


@pytest.mark.parametrize("t", [2.0 ** -24, 1.0 - 2.0 ** -24])
def test_brownian_at_the_ends_of_the_drawn_range(t):
    """t = 2^-24 is the smallest drawn u, 1 - 2^-24 the cap of every drawn t: gamma' is about 2^11 there, and finite."""
    eng, call, interp, s, g, c = _setup("vloss_ambient", "brownian")
    tv = np.full(g["x0"].shape[0], t, F32)
    assert float(tv[0]) == t and 0.0 < t < 1.0
    r = call(t=tv, z=c["z"], returns=ALL)
    assert np.isfinite(r["loss"]).all() and np.isfinite(r["mean"])
    _reduce_ok(r, g["x0"], g["x1"], _vn_kw(s))
    _reduce(f"brownian t {t!r}", r, g["x0"], g["x1"], _vn_kw(s))
    _stage_one(f"brownian t {t!r}", r["xt"], g["x0"], g["x1"], tv, c["z"], s["center"], **_vn_kw(s))


def test_sin2_accepts_the_closed_interval():
    eng, call, interp, s, g, c = _setup("vloss_ambient", "sin2")
    tv = np.asarray([0.0, 0.5, 1.0, 0.0, 1.0], F32)[: g["x0"].shape[0]]
    assert tv.shape[0] == g["x0"].shape[0]
    r = call(t=tv, z=c["z"], returns=ALL)
    assert np.isfinite(r["loss"]).all() and np.isfinite(r["mean"])
    _reduce_ok(r, g["x0"], g["x1"], _vn_kw(s))
    _reduce("sin2 t in {0, 0.5, 1}", r, g["x0"], g["x1"], _vn_kw(s))
    _stage_one("sin2 t in {0, 0.5, 1}", r["xt"], g["x0"], g["x1"], tv, c["z"], s["center"], **_vn_kw(s))


@pytest.mark.parametrize("a", [0.5, 40.0])
def test_sig_sum_at_a_flat_and_a_steep_parameter(a):
    eng, call, interp, s, g, c = _setup("vloss_ambient", "sig_sum")
    s = {**s, "a": a}
    r = call(a=a, t=c["t"], z=c["z"], returns=ALL)
    _reduce_ok(r, g["x0"], g["x1"], _vn_kw(s))
    _reduce(f"sig_sum a {a}", r, g["x0"], g["x1"], _vn_kw(s))
    _stage_one(f"sig_sum a {a}", r["xt"], g["x0"], g["x1"], c["t"], c["z"], s["center"], **_vn_kw(s))


# ------------------------------------------------------------------------------------------------ 4h. the first non-finite row
def test_the_first_non_finite_row_is_named_and_nothing_is_written():
    """TI_E_NAN (include/ti_hip.h): vloss_first_bad_kernel strides over B = 1000 rows with 256 threads and takes the minimum, so two bad
    rows given in descending order name the lower one, and a bad last row is found by the thread of the last, partial round.  The
    refusal is the documented one for non-finite arithmetic; no output is copied."""
    ti = pkg()
    eng, a = _adw_fixture()
    B = 1000
    x0, x1, b0, b1 = _adw_inputs(B, 8)
    bad = x1.copy()
    bad[[700, 300]] = np.inf
    with pytest.raises(ti._lib.TiError) as ei:
        eng.velocity_loss(x0, bad, b0, b1, a=a, seed=2)
    assert ei.value.code == ti._lib.TI_E_NAN and str(ei.value).endswith("molecule 300")
    desc = eng._vloss_desc("standard", "brownian", a, "none", None, "uniform", 2, 0, 0, 3)
    loss, mean, tb = np.full(B, 7.0), np.full(1, 7.0), np.full((3, 2), 7.0)
    t, z, xt, b = np.full(B, 7.0, F32), np.full(B, 7.0, F32), np.full((2, B), 7.0, F32), np.full((2, B), 7.0, F32)
    vp = lambda v: C.c_void_p(v.ctypes.data)
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    rc = ti._lib.lib().ti_adw_vloss(eng.h, C.byref(desc), vp(x0), vp(bad), vp(b0), vp(b1), None, None, B, vp(loss), dp(mean), dp(tb), vp(t), vp(z),
                                    vp(xt), vp(b), ti._lib.MEM_HOST)
    assert rc == ti._lib.TI_E_NAN and ti._lib.last_error().endswith("molecule 300")
    for out in (loss, mean, tb, t, z, xt, b):
        assert (out == 7.0).all()
    last = x1.copy()
    last[999] = np.inf
    with pytest.raises(ti._lib.TiError) as ei:
        eng.velocity_loss(x0, last, b0, b1, a=a, seed=2)
    assert ei.value.code == ti._lib.TI_E_NAN and str(ei.value).endswith("molecule 999")
    r = eng.velocity_loss(x0, x1, b0, b1, a=a, seed=2)                            # the handle is fine afterwards
    assert np.isfinite(r["loss"]).all()
