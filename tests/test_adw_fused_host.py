"""The fused adw rollout without a GPU: the export, its refusal of a NULL handle before any device call, and the register / scratch
guard of every adw_rollout_fused_kernel instantiation (code-object metadata only)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import ROOT, pkg

# adw_fused_kernels.hip: H in {32, 64, 128, 256} x {f32, f16x2} x {drift only, with tangent}; Heun is a run-time branch
N_FUSED_INSTANTIATIONS = 16


@pytest.fixture(scope="module")
def lib():
    ti = pkg()
    ti.build.build()
    return ti._lib.lib()


def test_fused_rollout_is_declared_listed_and_exported(lib):
    ti = pkg()
    assert "ti_adw_rollout_fused" in ti._lib.ABI_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "ti_hip.h")).read()
    assert re.search(r"int\s+ti_adw_rollout_fused\(ti_handle\* h, const ti_rollout_desc\* desc, const float\* x0, const float\* beta0, "
                     r"const float\* beta1,\s+int64_t B, float\* out_path, float\* out_dlogp[^,]*, int64_t\* n_fevals\);", hdr)
    assert hasattr(lib, "ti_adw_rollout_fused")
    assert lib.ti_version() == 5


def test_fused_rollout_refuses_a_null_handle(lib):
    ti = pkg()
    grid = np.linspace(0.0, 1.0, 4).astype(np.float32)
    rd = ti._lib.RolloutDesc(ti._lib.SCHEMES["euler"], grid.size, 1, ti._lib.MEM_HOST, 0.0, 0, 0, 0, ti._lib.fptr(grid), 0.0, 0.0, 0)
    x = np.zeros(4, np.float32)
    out = np.zeros((4, 4), np.float32)
    nfe = C.c_int64(-1)
    p = lambda a: C.c_void_p(a.ctypes.data)
    assert lib.ti_adw_rollout_fused(None, C.byref(rd), p(x), p(x), p(x), 4, p(out), None, C.byref(nfe)) == ti._lib.TI_E_ARG
    assert "adw handle" in ti._lib.last_error()
    assert nfe.value == -1 and not out.any()


def _llvm(name):
    p = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", name)
    return p if os.path.exists(p) else None


def test_every_fused_kernel_has_no_scratch_and_no_spills(lib):
    """Every adw_rollout_fused_kernel instantiation reports .private_segment_fixed_size 0, .sgpr_spill_count 0 and .vgpr_spill_count 0
    in its code-object metadata, and there are as many as adw_fused_kernels.hip documents."""
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
                m = re.search(r"\.name:\s+(\S*adw_rollout_fused_kernel\S*)", blk)
                if not m:
                    continue
                found[m.group(1)] = {k: int(re.search(rf"\.?{k}:\s+(\d+)", blk).group(1))
                                     for k in ("private_segment_fixed_size", "sgpr_spill_count", "vgpr_spill_count")}
    assert len(found) == N_FUSED_INSTANTIATIONS, sorted(found)
    assert not any("adw_mlp" in k for k in found), sorted(found)          # test_adw_nd_host.py counts the adw_mlp* kernels by name
    bad = {k: v for k, v in found.items() if any(v.values())}
    assert not bad, bad
