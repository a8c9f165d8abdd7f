"""Velocity loss, host side (no GPU): the ABI surface, the fp64 restatement against the reference fixtures, the refusals that return
before the device is touched, the driver's key checks, and the mirror classes' signatures."""
import ctypes as C
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

import vloss_numpy as vn
from conftest import ROOT, load_golden, pkg

NEW_SYMBOLS = ("ti_painn_vloss", "ti_adw_vloss", "ti_painn_vloss_interp", "ti_adw_vloss_interp")
U = 2.0 ** -53


@pytest.fixture(scope="module")
def lib():
    ti = pkg()
    ti.build.build()
    return ti._lib.lib()


def test_symbols_in_abi_list_library_and_header(lib):
    ti = pkg()
    hdr = open(os.path.join(ROOT, "include", "ti_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in ti._lib.ABI_SYMBOLS
        assert hasattr(lib, name)
        assert re.search(r"\bint " + name + r"\(ti_handle\* h, const ti_vloss_desc\* desc, ", hdr), name
    assert lib.ti_version() == 5
    assert "vloss_kernels.hip" in ti.build.SOURCES and "api_vloss.hip" in ti.build.SOURCES
    assert ti._lib.VLOSS_DOMAIN == vn.VLOSS_DOMAIN == int(re.search(r"#define TI_VLOSS_DOMAIN (0x[0-9a-f]+)u", hdr).group(1), 16)
    assert C.sizeof(ti._lib.VlossDesc) == 48


def _cases(name):
    g = load_golden(name)
    for case in g["cases"]:
        yield g, str(case), {k.split("::", 1)[1]: v for k, v in g.items() if k.startswith(f"{case}::")}


def _settings(name, g, case):
    """(kind, gamma, a, center) of a fixture case"""
    if name == "vloss_ambient":
        return "standard", case, float(g["a"][list(g["cases"]).index(case)]), "batch"
    if name == "vloss_latent_multi":
        return "one_sided", "brownian", 1.0, "batch"
    return case, "brownian", float(g["a"]), "none"


@pytest.mark.parametrize("name", ["vloss_ambient", "vloss_latent_multi", "vloss_adw_h64"])
def test_restatement_reproduces_the_reference_pieces(name):
    """The per-row loss and its mean from the fixture's own bt_plus / bt_minus within n_terms 2^-53 sum|terms|; the states within
    xt_ref_err S + 2^-24 S (the reference's measured fp32 error plus the rounding of the stored value)."""
    for g, case, c in _cases(name):
        kind, gamma, a, center = _settings(name, g, case)
        kw = dict(kind=kind, gamma_kind=gamma, a=a)
        mol = g["x0"].ndim == 3
        if mol:
            rows = vn.row_loss(g["x0"], g["x1"], c["t"], c["z"], c["bt_plus"], c["bt_minus"], **kw)
            f = lambda v: np.asarray(v, np.float64).reshape(-1, 3)
            _, mag, n_terms = vn.loss(f(g["x0"]), f(g["x1"]), np.repeat(c["t"], g["x0"].shape[1]), f(c["z"]), f(c["bt_plus"]), f(c["bt_minus"]), **kw)
        else:
            rows, mag, n_terms = vn.loss(g["x0"], g["x1"], c["t"], c["z"], c["bt_plus"], c["bt_minus"], **kw)
        assert rows.shape == c["row_loss"].shape
        assert (np.abs(rows - c["row_loss"]) <= n_terms * U * mag).all(), (name, case)
        n = rows.size
        assert abs(rows.mean() - float(c["mean"])) <= (n_terms + n) * U * mag.sum() / n, (name, case)
        xt, S = vn.interpolate(g["x0"], g["x1"], c["t"], c["z"], kind=kind, gamma_kind=gamma, a=a, center=center)
        ref = np.stack([c["xtp"], c["xtm"]])[: xt.shape[0]].astype(np.float64)
        assert (np.abs(xt - ref) <= (float(c["xt_ref_err"]) + 2.0 ** -24) * S).all(), (name, case)
        assert float(c["xt_ref_err"]) < 1e-6                                   # an fp32 chain: a few units of 2^-24


def _desc(ti, **kw):
    d = dict(kind=0, gamma=0, a=0.9, center=0, t_dist=1, seed=0, traj_offset=0, draw=0, n_tbins=0)
    d.update(kw)
    return ti._lib.VlossDesc(*(d[k] for k in ("kind", "gamma", "a", "center", "t_dist", "seed", "traj_offset", "draw", "n_tbins")))


def test_refusals_return_before_the_device_is_touched(lib):
    """Every TI_E_ARG case of include/ti_hip.h, on a machine without a GPU: the checks that need no handle come first and name what they
    refuse; the handle (NULL here) is refused last."""
    ti = pkg()
    E = ti._lib.TI_E_ARG
    x = np.zeros((2, 3, 3), np.float32)
    out = np.zeros(2, np.float64)
    p = lambda a: None if a is None else a.ctypes.data

    def painn(desc, t=None, z=None, B=2, mem=0, h=None):
        rc = lib.ti_painn_vloss(h, None if desc is None else C.byref(desc), p(x), p(x), p(x), p(t), p(z), B, p(out), None, None, None, None, None,
                                None, mem)
        return rc, lib.ti_last_error().decode()

    def adw(desc, t=None, z=None, B=2):
        rc = lib.ti_adw_vloss(None, C.byref(desc), p(x), p(x), p(x), p(x), p(t), p(z), B, p(out), None, None, None, None, None, None, 0)
        return rc, lib.ti_last_error().decode()

    def interp(desc, t=None, z=None, B=2):
        rc = lib.ti_painn_vloss_interp(None, C.byref(desc), p(x), p(x), p(t), p(z), B, None, None, p(x), 0)
        return rc, lib.ti_last_error().decode()

    half = np.asarray([0.5, 0.5], np.float32)
    for call in (painn, adw, interp):
        assert call(_desc(ti)) == (E, "not a painn handle" if call is not adw else "not an adw handle")          # everything else is in order
        for bad, word in ((dict(kind=2), "loss kind"), (dict(gamma=3), "gamma kind"), (dict(gamma=-1), "gamma kind"), (dict(center=3), "center"),
                          (dict(t_dist=4), "time distribution"), (dict(a=0.0), "must be finite and > 0"), (dict(a=-1.0, gamma=2), "must be finite and > 0"),
                          (dict(a=float("nan")), "must be finite and > 0"), (dict(n_tbins=-1), "n_tbins"), (dict(n_tbins=1025), "n_tbins")):
            rc, msg = call(_desc(ti, **bad))
            assert rc == E and word in msg, (bad, msg)
        assert call(_desc(ti, a=0.0, gamma=1))[1].startswith("not a")                   # sin2 does not use a
        assert call(_desc(ti, a=0.0, kind=1))[1].startswith("not a")                    # nor does the one-sided loss
        rc, msg = call(_desc(ti), B=0)
        assert rc == E and "B < 1" in msg
        rc, msg = call(_desc(ti, kind=1), z=x)
        assert rc == E and "z must be NULL" in msg
        rc, msg = call(_desc(ti, t_dist=0))
        assert rc == E and "needs t" in msg
        rc, msg = call(_desc(ti), t=half)
        assert rc == E and "t must be NULL" in msg
        for tv, word in (([0.5, 1.5], "t[1] is outside"), ([-0.1, 0.5], "t[0] is outside"), ([0.5, float("nan")], "t[1] is outside"),
                         ([0.0, 0.5], "t[0] is 0 or 1"), ([0.5, 1.0], "t[1] is 0 or 1")):
            rc, msg = call(_desc(ti, t_dist=0), t=np.asarray(tv, np.float32))
            assert rc == E and word in msg, (tv, msg)
        # the ends are fine where gamma' is finite there
        assert call(_desc(ti, t_dist=0, gamma=1), t=np.asarray([0.0, 1.0], np.float32))[1].startswith("not a")
        assert call(_desc(ti, t_dist=0, kind=1), t=np.asarray([0.0, 1.0], np.float32))[1].startswith("not a")
    rc, msg = painn(None)
    assert rc == E and "desc is NULL" in msg
    rc, msg = painn(_desc(ti), mem=7)
    assert rc == E and "unknown mem" in msg


def _config(tmp_path, **kw):
    d = dict(gamma="brownian", t_distr="uniform", interpolant_a=0.9, n_draws=2, tbins=4, seed=3, data_save_path=str(tmp_path / "out"),
             data_save_name="x")
    d.update(kw)
    return types.SimpleNamespace(**d)


@pytest.mark.parametrize("bad", [dict(gamma="cubic"), dict(t_distr="normal"), dict(interpolant_a=0.0), dict(interpolant_a="1"), dict(n_draws=0),
                                 dict(n_draws=1.5), dict(tbins=-1), dict(tbins=2000), dict(center="atom"), dict(seed=-1),
                                 dict(data_save_name="")])
def test_driver_refuses_malformed_keys_before_anything_else(tmp_path, bad):
    ti = pkg()

    class Boom:                                   # any use of the model would be device work
        def __getattr__(self, k):
            raise AssertionError("the model was touched")

    with pytest.raises(ValueError):
        ti.drivers.score_checkpoints(_config(tmp_path, **bad), Boom(), [(None, None, None, None)], [{}])
    assert not os.path.exists(tmp_path / "out")


def test_mirror_signatures_and_gamma_dot():
    ti = pkg()
    th = ti.thermo
    for mod in (th.ambient, th.latent, th.adw):                                   # the reference's import paths, attribute access
        assert mod.interpolants is th.interpolants and mod.losses is th.losses
    I, Ls = th.interpolants, th.losses
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values() if p.name != "self"]
    assert sig(I.LinearInterpolant.__init__) == [("a", 1), ("gamma", "brownian")]
    assert sig(I.OneSidedLinearInterpolant.__init__) == []
    assert sig(Ls.StandardVelocityLoss.__init__) == [("interpolant", inspect.Parameter.empty), ("t_distr", "uniform")]
    assert sig(Ls.OneSidedVelocityLoss.__init__) == [("interpolant", inspect.Parameter.empty), ("t_distr", "uniform")]
    with pytest.raises(NotImplementedError):
        I.LinearInterpolant(1.0, "cubic")
    with pytest.raises(AssertionError):
        Ls.StandardVelocityLoss(I.LinearInterpolant(), t_distr="normal")
    x0, x1 = np.asarray([[1.0, 2.0]]), np.asarray([[3.0, -1.0]])
    for gamma, a in (("brownian", 0.9), ("sin2", 1.0), ("sig_sum", 4.0)):
        ip = I.LinearInterpolant(a, gamma)
        for t in (0.1, 0.5, 0.9):
            h = 1e-6
            fd = (ip.gamma(t + h) - ip.gamma(t - h)) / (2 * h)
            assert abs(fd - ip.gamma_dot(t)) < 1e-8 * max(1.0, abs(fd)) + 1e-9, (gamma, t)                 # O(h^2) truncation, h = 1e-6
            a32 = float(np.float32(a))                                            # the mirror holds a as the reference does: float32
            assert abs(ip.gamma(t) - vn.gamma(gamma, a32, t)) < 1e-15 and abs(ip.gamma_dot(t) - vn.gamma_dot(gamma, a32, t)) < 1e-14
            assert np.allclose(ip.It(t, x0, x1), (1 - t) * x0 + t * x1, rtol=0, atol=1e-15)
            assert np.array_equal(ip.dtIt(t, x0, x1), x1 - x0)


def test_time_draws_stay_inside_the_open_interval():
    """The restated draws (what the GPU tests hold the kernel to): u is exact in float32 and never 0 or 1; the three maps stay in (0, 1)."""
    u = vn.draw_u(5, 0, 0, 4096)
    assert u.dtype == np.float32 and (u > 0).all() and (u < 1).all()
    assert np.array_equal((u.astype(np.float64) * 2.0 ** 24) % 2, np.ones(4096))           # odd multiples of 2^-24
    assert not np.array_equal(u, vn.draw_u(5, 0, 1, 4096)) and np.array_equal(u[7:], vn.draw_u(5, 7, 0, 4089))
    for dist in ("uniform", "beta_half", "beta_2_1"):
        t = vn.draw_t(dist, 5, 0, 0, 4096)
        assert (t > 0).all() and (t < 1).all()


# ------------------------------------------------------------------------------------------------ the Philox normal of the drawn z
NORMAL_C = r"""
#include "vloss_normal.hpp"
/* entries of the normal's whole input domain -- the 2^24 values of u1, the 2^24 angles 2 pi u2 -- at which the restated logf / sinf /
   cosf (and the rounded fp64 sqrt against sqrtf) differ from the host libm */
void vl_domain_mismatches(long out[4])
{
    out[0] = out[1] = out[2] = out[3] = 0;
    for (uint32_t k = 0; k < (1u << 24); ++k) {
        const float u = vl_uniform24(k << 8), a = 6.283185307179586f * u, l = logf(u), x = -2.0f * l;
        out[0] += vl_host_logf(u) != l;
        out[1] += vl_host_sincosf(a, 0) != sinf(a);
        out[2] += vl_host_sincosf(a, 1) != cosf(a);
        out[3] += (float)sqrt((double)x) != sqrtf(x);
    }
}
float vl_normal_words(uint32_t w1, uint32_t w2, int odd) { return vl_box_muller(w1, w2, odd); }
"""


@pytest.fixture(scope="module")
def normal_lib(tmp_path_factory):
    """csrc/vloss_normal.hpp compiled for the host, as plain C with contraction off (what the device build's pragma does)"""
    ti = pkg()
    d = tmp_path_factory.mktemp("vl_normal")
    src, so = d / "vl_normal.c", d / "libvl_normal.so"
    src.write_text(NORMAL_C)
    subprocess.check_call([os.environ.get("CC", "gcc"), "-O2", "-ffp-contract=off", "-fno-builtin", "-shared", "-fPIC", "-I", ti.build.CSRC,
                           "-o", str(so), str(src), "-lm"])
    L = C.CDLL(str(so))
    L.vl_normal_words.restype = C.c_float
    L.vl_normal_words.argtypes = [C.c_uint32, C.c_uint32, C.c_int]
    return L


def test_restated_libm_equals_the_host_libm_over_the_whole_domain(normal_lib):
    """The drawn z is oracle.normal bit for bit because vloss_normal.hpp restates the host libm's logf / sinf / cosf: over every argument
    the normal can see, none differs."""
    out = (C.c_long * 4)()
    normal_lib.vl_domain_mismatches(out)
    assert list(out) == [0, 0, 0, 0]


def test_box_muller_on_philox_words_equals_oracle_normal(normal_lib):
    """vl_box_muller on the Philox words of ti_normal's counter (trajectory, step, component / 4; key = seed) is oracle.normal."""
    from oracle import oracle
    seed = 0x1234567890
    trajs, steps, comps = np.arange(5, 37, dtype=np.uint64), (0, 3, 1000), np.arange(54)
    for step in steps:
        for comp in comps:
            ctr = np.stack([trajs & np.uint64(0xFFFFFFFF), trajs >> np.uint64(32), np.full(trajs.size, step, np.uint64),
                            np.full(trajs.size, comp >> 2, np.uint64)], axis=-1)
            o = vn.philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
            pair = (comp & 3) >> 1
            for i, tr in enumerate(trajs):
                got = normal_lib.vl_normal_words(int(o[i, 2 * pair]), int(o[i, 2 * pair + 1]), int(comp & 1))
                assert got == np.float32(oracle.normal(seed, int(tr), step, int(comp))), (tr, step, comp)


# ------------------------------------------------------------------------------------------------ the fixed summation order
def _tree_loop(sm):
    s = 128
    while s:
        for i in range(s):
            sm[i] += sm[i + s]
        s >>= 1
    return sm[0]


def _colsum_loop(v):
    """vloss_tile_sum_kernel and vloss_tile_combine_kernel with ncol = 1, thread by thread"""
    n, tiles = len(v), max(1, -(-len(v) // 1024))
    partial = []
    for tile in range(tiles):
        sm = [0.0] * 256
        for j in range(256):
            for k in range(4):
                r = tile * 1024 + 4 * j + k
                if r < n:
                    sm[j] += v[r]
        partial.append(_tree_loop(sm))
    sm = [0.0] * 256
    for j in range(256):
        for k in range(j, tiles, 256):
            sm[j] += partial[k]
    return _tree_loop(sm)


def _sixteen_decades(n, seed):
    rs = np.random.RandomState(seed)
    return rs.standard_normal(n) * 10.0 ** rs.uniform(-8.0, 8.0, n)


@pytest.mark.parametrize("n", [1, 255, 1024, 1025, 2500, 265145])
def test_fixed_order_sum_is_the_kernels_loop_and_close_to_fsum(n):
    """The vectorised restatement against the scalar transcription of the two kernels, bit for bit, on values spread over 16 decades
    (any other association shows); and against the exact sum within the bound of ANY order, (n - 1) 2^-53 sum|v|."""
    import math
    v = _sixteen_decades(n, n)
    got = vn.fixed_order_sum(v)
    assert got == _colsum_loop(v.tolist())
    bound = (n - 1) * U * np.abs(v).sum()
    print(f"fixed_order_sum n {n}: |sum - fsum| / (2^-53 sum|v|) {abs(got - math.fsum(v)) / (U * np.abs(v).sum()):.3f}")
    assert abs(got - math.fsum(v)) <= bound
    assert vn.fixed_order_sum(np.concatenate([v, np.zeros(3)])) == got           # +0.0 rows are not seen: padding is skipping


@pytest.mark.parametrize("n", [1, 7, 1024])
def test_time_bins_fixed_order_against_time_bins(n):
    B = 2500
    l = _sixteen_decades(B, 77)
    t = np.random.RandomState(78).uniform(0.0, 1.0, B).astype(np.float32)
    t[:3] = (0.0, 1.0, vn.T_MAX)
    got, ref = vn.time_bins_fixed_order(l, t, n), vn.time_bins(l, t, n)
    assert got.shape == (n, 2) and np.array_equal(got[:, 1], ref[:, 1]) and got[:, 1].sum() == B
    assert (np.abs(got[:, 0] - ref[:, 0]) <= B * U * np.abs(l).sum()).all()
    k = np.minimum(np.floor(t.astype(np.float64) * n).astype(int), n - 1)                # vloss_tbins_kernel, thread by thread, on a few bins
    for b in sorted({0, n // 2, n - 1}):
        sm = [0.0] * 256
        for j in range(256):
            for i in range(j, B, 256):
                if k[i] == b:
                    sm[j] += l[i]
        assert got[b, 0] == _tree_loop(sm)


@pytest.mark.parametrize("B,A", [(513, 2), (171, 6)])
def test_dyadic_construction_is_exact_in_fp64(B, A):
    """What the bit-for-bit centring tests of tests/test_gpu_vloss_edges.py rest on, in rational arithmetic: on dyadic_case the one-sided
    state t x1 + (1 - t) x0 and its column sums are exact in fp64 (so they are the same in any order and under any contraction),
    colsum / rows is the one correctly rounded division, and raw - mean is the correctly rounded difference of those two numbers."""
    from fractions import Fraction as Fr
    x0, x1, t = vn.dyadic_case(B, A, seed=B)
    raw = vn.interpolate(x0, x1, t, kind="one_sided", center="none")[0][0]
    exact = [[Fr(float(t[b])) * Fr(float(c1)) + (1 - Fr(float(t[b]))) * Fr(float(c0)) for c0, c1 in zip(x0[b].reshape(-1), x1[b].reshape(-1))] for b in range(B)]
    assert all(Fr(float(r)) == e for rb, eb in zip(raw.reshape(B, -1), exact) for r, e in zip(rb, eb))
    rows = B * A
    cols = [sum(eb[3 * a + c] for eb in exact for a in range(A)) for c in range(3)]
    flat = raw.reshape(rows, 3)
    for c in range(3):
        assert Fr(float(flat[:, c].sum())) == cols[c] and Fr(vn.fixed_order_sum(flat[:, c])) == cols[c] and Fr(float(flat[::-1, c].sum())) == cols[c]
    mean = flat.sum(axis=0) / rows
    assert all(float(mean[c]) == float(cols[c] / rows) for c in range(3))                # Fraction -> float rounds correctly
    xt = vn.interpolate(x0, x1, t, kind="one_sided", center="batch")[0][0].reshape(rows, 3)
    assert np.array_equal(xt, flat - mean)
    for r in range(0, rows, 7):
        for c in range(3):
            assert float(xt[r, c]) == float(Fr(float(flat[r, c])) - Fr(float(mean[c])))
    mol = vn.interpolate(x0, x1, t, kind="one_sided", center="molecule")[0][0]
    for b in range(0, B, 5):
        for c in range(3):
            m = sum(exact[b][3 * a + c] for a in range(A)) / A
            assert all(float(mol[b, a, c]) == float(Fr(float(raw[b, a, c])) - Fr(float(m))) for a in range(A))


def test_interpolate_return_abs_leaves_existing_callers_alone():
    x0, x1, t = vn.dyadic_case(7, 2)
    z = np.random.RandomState(0).standard_normal(x0.shape)
    two = vn.interpolate(x0, x1, t, z)
    xt, S, E = vn.interpolate(x0, x1, t, z, return_abs=True)
    assert len(two) == 2 and np.array_equal(two[0], xt) and np.array_equal(two[1], S) and E.shape == (2, 3)
    raw = vn.interpolate(x0, x1, t, z, center="none")[0]
    assert np.allclose(E, np.abs(raw).reshape(2, -1, 3).sum(axis=1), rtol=1e-15)
    assert vn.interpolate(x0[:, 0, 0], x1[:, 0, 0], t, kind="one_sided", center="none", return_abs=True)[2].shape == (1,)
    assert vn.interpolate(x0[:, 0], x1[:, 0], t, kind="one_sided", center="none", return_abs=True)[2].shape == (1, 3)
