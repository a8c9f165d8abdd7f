"""FCNetMultiBeta in d dimensions, without a GPU: the new export, argument validation before any device call, the fp64 numpy
restatement against every d-dimensional fixture, and the register / scratch guard of every adw kernel instantiation."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from adw_nd_numpy import CASES, drift, load_case
from conftest import ROOT, pkg


@pytest.fixture(scope="module")
def lib():
    ti = pkg()
    ti.build.build()
    return ti._lib.lib()


def _create_nd(lib, H, L, dim, n_weights):
    ti = pkg()
    desc = ti._lib.AdwDesc(H, L, ti._lib.PRECISIONS["f32"])
    w = np.zeros(max(n_weights, 1), np.float64)
    return lib.ti_adw_create_nd(C.byref(desc), dim, w.ctypes.data_as(C.POINTER(C.c_double)), n_weights, 0)


def _n_weights(H, L, d):
    ti = pkg()
    return ti.weights.n_params(ti.weights.adw_param_spec(H, L, d, d))


def test_create_nd_is_exported_and_declared(lib):
    ti = pkg()
    assert "ti_adw_create_nd" in ti._lib.ABI_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "ti_hip.h")).read()
    assert re.search(r"ti_handle\*\s+ti_adw_create_nd\(const ti_adw_desc\* desc, int32_t dim, const double\* weights, size_t n_weights, "
                     r"int device\);", hdr)
    assert hasattr(lib, "ti_adw_create_nd")


@pytest.mark.parametrize("dim", [0, 17, -1])
def test_create_nd_refuses_dim_outside_1_16(lib, dim):
    ti = pkg()
    assert not _create_nd(lib, 64, 3, dim, _n_weights(64, 3, 2))
    assert "dim" in ti._lib.last_error()


@pytest.mark.parametrize("dim", [1, 2, 16])
def test_create_nd_refuses_wrong_weight_count(lib, dim):
    ti = pkg()
    n = _n_weights(64, 3, dim)
    for bad in (n - 1, n + 1, _n_weights(64, 3, dim % 16 + 1)):
        assert not _create_nd(lib, 64, 3, dim, bad)
        assert "weight count" in ti._lib.last_error() and str(n) in ti._lib.last_error()


def test_weight_count_formula():
    """1-D formula with the input layer H (d + 2) and the output layer d H + d (include/ti_hip.h weight layout)."""
    for H, L, d in ((32, 1, 1), (64, 3, 2), (256, 5, 16)):
        be = H * 3 + H + H * H + H + H + 1
        net = H * (d + 2) + H + (L - 1) * (H * H + H) + d * H + d
        assert _n_weights(H, L, d) == be + net


def test_fcnet_refuses_non_ode_and_large_d():
    adw = pkg().thermo.adw_nd
    with pytest.raises(ValueError, match="not an ODE"):
        adw.FCNetMultiBeta(2, 3, 64, 3)
    with pytest.raises(NotImplementedError, match="16"):
        adw.FCNetMultiBeta(17, 17, 64, 3)
    m = adw.FCNetMultiBeta(3, 3, 64, 3)
    assert m.dim == 3 and m.state_dict()["net.0.weight"].shape == (64, 5) and m.state_dict()["net.6.weight"].shape == (3, 64)


def test_one_dim_mirror_keeps_its_contract_and_points_to_nd():
    """thermo.adw keeps the reference sampler's 1-D contract; its refusal names the d-dimensional shell."""
    ti = pkg()
    with pytest.raises(NotImplementedError, match="adw_nd"):
        ti.thermo.adw.FCNetMultiBeta(2, 2, 64, 3)
    assert ti.thermo.adw_nd.ODEWrapper is ti.thermo.adw.ODEWrapper
    assert ti.thermo.adw_nd.StandardIntegrator is ti.thermo.adw.StandardIntegrator
    m = ti.thermo.adw_nd.FCNetMultiBeta(1, 1, 64, 3)
    assert m.dim == 1 and m.state_dict()["net.0.weight"].shape == (64, 3)


def test_from_torch_module_infers_d():
    torch = pytest.importorskip("torch")
    adw = pkg().thermo.adw_nd
    H, L, d = 32, 2, 4
    ti = pkg()

    class Fake:
        def state_dict(self):
            sd = ti.synthetic.make_state_dict(ti.weights.adw_param_spec(H, L, d, d), seed=3, dtype=np.float64)
            return {k: torch.from_numpy(v) for k, v in sd.items()}
    m = adw.FCNetMultiBeta.from_torch_module(Fake())
    assert (m.dim, m.hidden_size, m.num_layers) == (d, H, L)
    with pytest.raises(NotImplementedError, match="adw_nd"):
        pkg().thermo.adw.FCNetMultiBeta.from_torch_module(Fake())


def test_sample_adw_refuses_d_above_1():
    ti = pkg()
    m = ti.thermo.adw_nd.FCNetMultiBeta(2, 2, 32, 2)
    with pytest.raises(NotImplementedError, match="component 0"):
        ti.drivers.sample_adw(None, m, [])


@pytest.mark.parametrize("name", CASES)
def test_numpy_restatement_reproduces_fixture(name):
    g, sd = load_case(name)
    d = int(g["dim"])
    if "sd_abs_sum" in g:
        assert abs(sum(float(np.abs(v).sum()) for v in sd.values()) - float(g["sd_abs_sum"])) <= 1e-9 * float(g["sd_abs_sum"])
    x = g["x"]
    assert x.shape == (int(g["B"]), d)
    for tag, b0, b1 in (("", g["beta0"], g["beta1"]), ("_var", g["beta0_var"], g["beta1_var"])):
        times = [(str(i), t) for i, t in enumerate(g["ts"])] + [("tv", g["tv"])]
        for key, t in times:
            b, div = drift(sd, x, t, b0, b1, return_div=True)
            ref_b, ref_nd = g[f"drift{tag}_{key}"], g[f"negdiv{tag}_{key}"]
            assert np.abs(b - ref_b).max() <= 1e-12 * max(1.0, np.abs(ref_b).max()), (tag, key)
            assert np.abs(-div * 1e-2 - ref_nd).max() <= 1e-12 * max(1e-3, np.abs(ref_nd).max()), (tag, key)
    grid = g["traj_grid"].astype(np.float64)
    for scheme in ("euler", "heun"):
        xs, dl = x.copy(), np.zeros(x.shape[0])
        for k in range(len(grid) - 1):
            dt = np.float64(np.float32(grid[k + 1]) - np.float32(grid[k]))
            b1_, d1 = drift(sd, xs, grid[k], g["beta0"], g["beta1"], return_div=True)
            if scheme == "euler":
                xs, dl = xs + dt * b1_, dl - dt * d1 * 1e-2
            else:
                xp = xs + dt * b1_
                b2_, d2 = drift(sd, xp, grid[k + 1], g["beta0"], g["beta1"], return_div=True)
                xs, dl = xs + 0.5 * dt * (b1_ + b2_), dl - 0.5 * dt * (d1 + d2) * 1e-2
        assert np.abs(xs - g[f"traj_{scheme}"][-1]).max() <= 1e-12 * max(1.0, np.abs(xs).max()), scheme
        assert np.abs(dl * 1e2 - g[f"dlogp_{scheme}"][-1]).max() <= 1e-12 * max(1.0, np.abs(dl * 1e2).max()), scheme


# ------------------------------------------------------------------------------------------------ ISA guard
def _llvm(name):
    p = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", name)
    return p if os.path.exists(p) else None


def test_every_adw_kernel_has_no_scratch_and_no_spills(lib):
    """the F = 256 device fault came from SGPR lane spills.  Every adw_mlp_kernel / adw_mlp_nd_kernel instantiation
    must report .private_segment_fixed_size 0, .vgpr_spill_count 0 and .sgpr_spill_count 0 in its code-object metadata."""
    import test_build_isa as isa
    readelf = _llvm("llvm-readelf")
    if not readelf or not all(_llvm(t) for t in ("llvm-objcopy", "clang-offload-bundler")):
        pytest.skip("ROCm LLVM tools not found")
    so = os.path.join(ROOT, "thermodynamic-interpolation_amd", "libti_hip.so")
    found = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in isa.code_objects(so, tmp):
            notes = subprocess.run([readelf, "--notes", co], check=True, capture_output=True, text=True).stdout
            for blk in re.split(r"\n\s+- \.", notes):
                m = re.search(r"\.name:\s+(\S*adw_mlp\S*)", blk)
                if not m:
                    continue
                vals = {k: int(re.search(rf"\.?{k}:\s+(\d+)", blk).group(1))
                        for k in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count")}
                found[m.group(1)] = vals
    nd = [k for k in found if "adw_mlp_nd_kernel" in k]
    assert len(found) == 32 and len(nd) == 16, sorted(found)        # {H 32..256} x {f32, f16x2} x {drift, divergence} x {1-D, d-D}
    bad = {k: v for k, v in found.items() if any(v.values())}
    assert not bad, bad
