"""Thin Python objects over the C ABI handles (include/ti_hip.h).  No arithmetic happens here.

Buffers may be numpy arrays (host memory, staged by the library) or CUDA/HIP torch tensors (used in place through
``data_ptr()``; nothing from torch is imported in this module).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import weights as W


def time_grid(start: float, end: float, n_step: int) -> np.ndarray:
    """The reference grid ``torch.linspace(start, end, n_step)`` as float32
    (/root/reference/mdqm9/thermo/ambient/integrators.py:43).  PyTorch is used for it when importable, so the values are
    bit-identical to the reference's; otherwise the same two-sided formula is evaluated in numpy (within 1 ulp: torch's
    vectorised kernel rounds ``start + step * i`` in two stages)."""
    try:
        import torch
        return torch.linspace(float(start), float(end), int(n_step), dtype=torch.float32).numpy().copy()
    except ImportError:
        return _time_grid_numpy(start, end, n_step)


def _time_grid_numpy(start: float, end: float, n_step: int) -> np.ndarray:
    start, end = np.float32(start), np.float32(end)
    if n_step == 1:
        return np.asarray([start], np.float32)
    step = np.float32((end - start) / np.float32(n_step - 1))
    i = np.arange(n_step, dtype=np.int64)
    lo = start + step * i.astype(np.float32)
    hi = end - step * (n_step - 1 - i).astype(np.float32)
    return np.where(i < n_step // 2, lo, hi).astype(np.float32)


STEP_CONTROLS = ("batch", "trajectory")


def scheme_code(scheme, step_control="batch"):
    """TI_SCHEME_* of a scheme name.  step_control: 'batch' (one step size for the whole call, torchdiffeq's odeint per mini-batch)
    or 'trajectory' (dopri5 only: every trajectory gets the steps a batch of one would take -- TI_SCHEME_DOPRI5_TRAJ)."""
    if step_control not in STEP_CONTROLS:
        raise ValueError(f"unknown step_control {step_control!r}; expected one of {STEP_CONTROLS}")
    if isinstance(scheme, str):
        if scheme not in _lib.SCHEMES:
            raise ValueError(f"unknown scheme {scheme!r}; expected one of {sorted(_lib.SCHEMES)}")
        scheme = _lib.SCHEMES[scheme]
    if step_control == "trajectory":
        if scheme != _lib.SCHEMES["dopri5"]:
            raise ValueError("step_control='trajectory' needs the adaptive scheme 'dopri5'")
        scheme = _lib.SCHEME_DOPRI5_TRAJ
    return scheme


def _rollout_desc(scheme, t_grid, save_every, mem, eps, seed, traj_offset, com_free_noise, rtol=0.0, atol=0.0, step_offset=0,
                  step_control="batch"):
    t_grid = np.ascontiguousarray(t_grid, np.float32)
    if t_grid.ndim != 1 or t_grid.size < 1:
        raise ValueError("t_grid must be a non-empty 1-D array")
    scheme = scheme_code(scheme, step_control)
    rd = _lib.RolloutDesc(scheme, t_grid.size, int(save_every), mem, float(eps), int(bool(com_free_noise)), int(seed),
                          int(traj_offset), _lib.fptr(t_grid), float(rtol), float(atol), int(step_offset))
    rd._keep = t_grid
    return rd


def _alloc_like(template, shape):
    """Output buffer living where `template` lives (numpy -> numpy, cuda tensor -> cuda tensor)."""
    if hasattr(template, "data_ptr"):
        return template.new_empty(shape)
    return np.empty(shape, np.float32)


class _Engine:
    h = None
    device = 0

    def close(self):
        if self.h:
            _lib.lib().ti_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream: int | None, external: bool = True):
        """Run on the caller's HIP stream (`hip_stream` = hipStream_t as int; 0 / None = the null stream, which is what torch's
        default stream reports), or with external=False on the handle's own stream again."""
        _lib.check(_lib.lib().ti_set_stream(self.h, C.c_void_p(hip_stream or 0), 1 if external else 0))

    def wait_stream(self, hip_stream: int | None):
        """Order the handle's stream after everything enqueued so far on `hip_stream` (0 / None = the null stream)."""
        _lib.check(_lib.lib().ti_wait_stream(self.h, C.c_void_p(hip_stream or 0)))

    def _ptrs(self, *specs):
        """as_ptr over (buffer, shape, is_output, name) specs; all present buffers must live in one memory space.  Device buffers
        must be on this engine's GPU, and the handle's stream is ordered after torch's current stream on that GPU first, so a
        tensor produced by a still-running torch kernel is never read early.  Returns (pointers, is_device, keepalives)."""
        ptrs, keep, spaces, devs = [], [], set(), set()
        for buf, shape, out, what in specs:
            pt, k, dev, idx = _lib.as_ptr(buf, shape=shape, out=out, what=what)
            ptrs.append(pt); keep.append(k)
            if buf is not None:
                spaces.add(dev)
                if idx is not None:
                    devs.add(idx)
        if len(spaces) > 1:
            raise ValueError("all buffers of a call must live in the same memory space (all host or all on the GPU)")
        dev = bool(spaces and spaces.pop())
        if dev:
            if devs - {self.device}:
                raise ValueError(f"tensors live on cuda:{sorted(devs)} but this engine was created on device {self.device}")
            if devs:                                  # torch tensors (raw int addresses carry no stream: the caller orders them)
                import torch
                self.wait_stream(torch.cuda.current_stream(self.device).cuda_stream)
        return ptrs, dev, keep

    def reserve(self, B: int):
        _lib.check(_lib.lib().ti_reserve(self.h, int(B)))

    def profile(self, on: bool = True):
        _lib.check(_lib.lib().ti_profile_enable(self.h, int(on)))

    def profile_read(self, kernel: str):
        n, ms = C.c_int64(0), C.c_double(0.0)
        _lib.check(_lib.lib().ti_profile_read(self.h, _lib.KERNELS[kernel], C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def step_counts(self, B: int):
        """(accepted [B], rejected [B]) int64 step counts of every trajectory of the last step_control='trajectory' rollout."""
        acc, rej = np.zeros(int(B), np.int64), np.zeros(int(B), np.int64)
        p = C.POINTER(C.c_int64)
        _lib.check(_lib.lib().ti_rollout_step_counts(self.h, acc.ctypes.data_as(p), rej.ctypes.data_as(p), int(B)))
        return acc, rej

    # ---- observables (include/ti_hip.h ti_obs_*; the user-facing functions and the descriptor syntax are in observables.py)
    def _obs_n_atoms(self):
        return getattr(self, "A", 1)

    def _obs_args(self, descriptors, ref, select):
        from . import observables as _obs
        desc = _obs.encode_descriptors(descriptors)
        A = self._obs_n_atoms()
        host = lambda a: a.detach().cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)
        r = sel = None
        if ref is not None:
            r = np.ascontiguousarray(host(ref), np.float32)
            if r.shape != (A, 3):
                raise ValueError(f"ref must be [{A},3], got {r.shape}")
        if select is not None:
            sel = np.ascontiguousarray(host(select) != 0, np.int32)
            if sel.shape != (A,):
                raise ValueError(f"select must be [{A}], got {sel.shape}")
        ptr = lambda a, f: None if a is None else f(a)
        return desc, r, sel, (_lib.iptr(desc), int(desc.shape[0]), ptr(r, _lib.fptr), ptr(sel, _lib.iptr))

    def _obs_x_shape(self, x):
        raise NotImplementedError

    def collective_variables(self, x, descriptors, ref=None, select=None, out=None):
        """cv [B, K] float32 of the K descriptors (observables.encode_descriptors) on x; computed on the GPU in fp64.  x: numpy or a
        CUDA tensor (the result lives where x lives)."""
        desc, r, sel, (dp, K, rp, sp) = self._obs_args(descriptors, ref, select)
        B, xs = self._obs_x_shape(x)
        if out is None:
            out = _alloc_like(x if hasattr(x, "data_ptr") and x.is_cuda else None, (B, K))
        (xp, op), dev, keep = self._ptrs((x, xs, False, "x"), (out, (B, K), True, "out"))
        _lib.check(_lib.lib().ti_obs_cv(self.h, dp, K, rp, sp, xp, B, op, _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        return out

    def importance_weights(self, logw):
        """(w [B] float32 = exp(logw) / sum exp(logw), ess) with a max shift and fixed-order fp64 sums; a non-finite logw raises."""
        B = int(logw.shape[0])
        w = _alloc_like(logw if hasattr(logw, "data_ptr") and logw.is_cuda else None, (B,))
        (lp, wp), dev, keep = self._ptrs((logw, (B,), False, "logw"), (w, (B,), True, "out_w"))
        ess = C.c_double(0.0)
        _lib.check(_lib.lib().ti_obs_weights(self.h, lp, B, wp, C.byref(ess), _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        return w, ess.value

    def bootstrap(self, logw, estimator, filter=0, k=1.0, level=0.95, n_boot=1000, first=0, seed=0, indices=None, out_boot=None):
        """ti_obs_bootstrap: (point, lower, upper, n_kept, estimates [n_boot] float64) of the estimator / filter codes (TI_BOOT_*) on
        logw [n] float32.  indices [n_boot, n_draw] int32: explicit population indices instead of the generator's draws.  logw numpy:
        indices numpy, estimates numpy; logw a CUDA tensor: indices a CUDA int32 tensor, estimates a CUDA float64 tensor."""
        n, n_boot = int(logw.shape[0]), int(n_boot)
        dev_in = hasattr(logw, "data_ptr") and logw.is_cuda
        n_draw, ip, keep_i = 0, None, None
        if indices is not None:
            if tuple(indices.shape[:1]) != (n_boot,) or len(indices.shape) != 2:
                raise ValueError(f"indices must be [n_boot = {n_boot}, n_draw], got {tuple(indices.shape)}")
            n_draw = int(indices.shape[1])
            if dev_in:
                if not (hasattr(indices, "data_ptr") and indices.is_cuda and str(indices.dtype) == "torch.int32" and indices.is_contiguous()):
                    raise TypeError("indices must be a contiguous CUDA int32 tensor when logw is a CUDA tensor")
                if (indices.device.index or 0) != self.device:
                    raise ValueError(f"indices live on {indices.device} but this engine was created on device {self.device}")
                keep_i, ip = indices, C.c_void_p(indices.data_ptr())
            else:
                if hasattr(indices, "data_ptr"):
                    indices = indices.detach().cpu().numpy()
                keep_i = np.ascontiguousarray(indices, np.int32)
                ip = C.c_void_p(keep_i.ctypes.data)
        if out_boot is None and n_boot > 0:
            if dev_in:
                import torch
                out_boot = torch.empty(n_boot, dtype=torch.float64, device=logw.device)
            else:
                out_boot = np.empty(n_boot, np.float64)
        bp = None
        if out_boot is not None:
            bp = C.c_void_p(out_boot.data_ptr() if hasattr(out_boot, "data_ptr") else out_boot.ctypes.data)
        (lp,), dev, keep = self._ptrs((logw, (n,), False, "logw"))
        desc = _lib.BootDesc(int(estimator), int(filter), float(k), float(level), n_boot, int(first), int(seed) & 0xFFFFFFFFFFFFFFFF)
        out = (C.c_double * 4)()
        _lib.check(_lib.lib().ti_obs_bootstrap(self.h, lp, n, C.byref(desc), ip, n_draw, out, bp, _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        return out[0], out[1], out[2], int(out[3]), out_boot

    def rff_gram_wide(self, values, omega, logw=None, n_boot=0, first=0, seed=0, indices=None, n_draw=0):
        """ti_obs_rff_gram_wide: ``rff_gram`` for p <= 1024 (beyond 128 columns the blocked pass); the same arguments and result."""
        return self.rff_gram(values, omega, logw, n_boot, first, seed, indices, n_draw, _entry="ti_obs_rff_gram_wide")

    def rff_gram(self, values, omega, logw=None, n_boot=0, first=0, seed=0, indices=None, n_draw=0, _entry="ti_obs_rff_gram"):
        """ti_obs_rff_gram: G [1 + n_boot, p, p] complex128 of values [n] or [n, d] float32 (numpy, or a CUDA tensor -- a view with
        unit stride along d, such as cv[:, :2], is read in place) and omega [d, p] float64 (host).  Row 0 is the point estimate, row
        1 + r resample first + r of the stream `seed`, or row r of indices [n_boot, n_draw] int32.  Lives where values lives."""
        n_boot, n_draw = int(n_boot), int(n_draw)
        om = np.ascontiguousarray(omega, np.float64)
        if om.ndim != 2:
            raise ValueError(f"omega must be [d, p], got {om.shape}")
        d, p = om.shape
        if len(values.shape) not in (1, 2) or (len(values.shape) == 2 and int(values.shape[1]) != d) or (len(values.shape) == 1 and d != 1):
            raise ValueError(f"values must be [n, d = {d}] (or [n] with d = 1), got {tuple(values.shape)}")
        n = int(values.shape[0])
        dev_in = hasattr(values, "data_ptr") and values.is_cuda
        if dev_in:
            if str(values.dtype) != "torch.float32":
                raise TypeError(f"values must be float32, got {values.dtype}")
            if len(values.shape) == 2 and d > 1 and values.stride(1) != 1:
                raise ValueError("values must have unit stride along d")
            if (values.device.index or 0) != self.device:
                raise ValueError(f"values live on {values.device} but this engine was created on device {self.device}")
            stride = max(int(values.stride(0)), d) if n > 1 else d
            keep_v, vp = values, C.c_void_p(values.data_ptr())
        else:
            host = values.detach().cpu().numpy() if hasattr(values, "data_ptr") else values
            keep_v = np.ascontiguousarray(np.asarray(host, np.float32).reshape(n, d))
            stride, vp = d, C.c_void_p(keep_v.ctypes.data)
        ip, keep_i = None, None
        if indices is not None:
            if tuple(indices.shape[:1]) != (n_boot,) or len(indices.shape) != 2:
                raise ValueError(f"indices must be [n_boot = {n_boot}, n_draw], got {tuple(indices.shape)}")
            n_draw = int(indices.shape[1])
            if dev_in:
                if not (hasattr(indices, "data_ptr") and indices.is_cuda and str(indices.dtype) == "torch.int32" and indices.is_contiguous()):
                    raise TypeError("indices must be a contiguous CUDA int32 tensor when values is a CUDA tensor")
                keep_i, ip = indices, C.c_void_p(indices.data_ptr())
            else:
                if hasattr(indices, "data_ptr"):
                    indices = indices.detach().cpu().numpy()
                keep_i = np.ascontiguousarray(indices, np.int32)
                ip = C.c_void_p(keep_i.ctypes.data)
        (lp,), ldev, keep = self._ptrs((logw, (n,), False, "logw"))
        if logw is not None and ldev != dev_in:
            raise ValueError("all buffers of a call must live in the same memory space (all host or all on the GPU)")
        if dev_in:
            import torch
            self.wait_stream(torch.cuda.current_stream(self.device).cuda_stream)
            out = torch.empty((1 + n_boot, p, p, 2), dtype=torch.float64, device=values.device)
            op = C.c_void_p(out.data_ptr())
        else:
            out = np.empty((1 + n_boot, p, p, 2), np.float64)
            op = C.c_void_p(out.ctypes.data)
        desc = _lib.GramDesc(d, p, n_boot, int(first), int(seed) & 0xFFFFFFFFFFFFFFFF)
        _lib.check(getattr(_lib.lib(), _entry)(self.h, vp, stride, n, om.ctypes.data_as(C.POINTER(C.c_double)), lp, C.byref(desc), ip, n_draw, op,
                                               _lib.MEM_DEVICE if dev_in else _lib.MEM_HOST))
        if dev_in:
            import torch
            return torch.view_as_complex(out)
        return out.view(np.complex128)[..., 0]

    def _complex_stack(self, a, what):
        """(pointer, keepalive, is_device, shape) of a stack of complex128 matrices [.., n, n]: numpy (any dtype that converts), or a
        contiguous CUDA complex128 tensor on this engine's GPU, read in place as (re, im) pairs."""
        if hasattr(a, "data_ptr") and a.is_cuda:
            if str(a.dtype) != "torch.complex128" or not a.is_contiguous():
                raise TypeError(f"{what} must be a contiguous complex128 tensor, got {a.dtype}")
            if (a.device.index or 0) != self.device:
                raise ValueError(f"{what} lives on {a.device} but this engine was created on device {self.device}")
            import torch
            self.wait_stream(torch.cuda.current_stream(self.device).cuda_stream)
            return C.c_void_p(a.data_ptr()), a, True, tuple(a.shape)
        host = np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "data_ptr") else a, np.complex128)
        return C.c_void_p(host.ctypes.data), host, False, host.shape

    def _eig_out(self, like, shape, dtype):
        """An output of ti_obs_eigh / ti_obs_gedmd_spectrum where the input lives: (array or tensor, pointer)"""
        if like is not None:
            import torch
            out = torch.empty(shape, dtype=getattr(torch, dtype), device=like.device)
            return out, C.c_void_p(out.data_ptr())
        out = np.empty(shape, getattr(np, dtype))
        return out, C.c_void_p(out.ctypes.data)

    def eigh(self, a, vectors=True, _entry="ti_obs_eigh", _max_n=_lib.EIGH_MAX_N):
        """ti_obs_eigh: (w [.., n] float64 ascending, v [.., n, n] complex128 or None, sweeps [..] int32) of a stack a [.., n, n] of
        Hermitian matrices, n <= 64, as numpy.linalg.eigh(a, UPLO="U"): parallel cyclic Jacobi, one workgroup per matrix.  Lives
        where a lives (numpy, or a CUDA complex128 tensor)."""
        ap, keep, dev, shape = self._complex_stack(a, "a")
        if len(shape) < 2 or shape[-1] != shape[-2] or not 1 <= shape[-1] <= _max_n:
            raise ValueError(f"a must be [.., n, n] with 1 <= n <= {_max_n}, got {tuple(shape)}")
        n, lead = int(shape[-1]), tuple(shape[:-2])
        n_mat = int(np.prod(lead, dtype=np.int64))
        if not 1 <= n_mat <= _lib.EIGH_MAX_MATRICES:
            raise ValueError(f"a must hold 1..{_lib.EIGH_MAX_MATRICES} matrices, got {n_mat}")
        like = keep if dev else None
        w, wp = self._eig_out(like, (*lead, n), "float64")
        v, vp = self._eig_out(like, (*lead, n, n, 2), "float64") if vectors else (None, None)
        sw, sp = self._eig_out(like, lead, "int32")
        _lib.check(getattr(_lib.lib(), _entry)(self.h, ap, n_mat, n, wp, vp, sp, _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        if v is not None:
            if dev:
                import torch
                v = torch.view_as_complex(v)
            else:
                v = v.view(np.complex128)[..., 0]
        return w, v, sw

    def eigh_wide(self, a, vectors=True):
        """ti_obs_eigh_wide: ``eigh`` for n <= 1024.  n <= 64 returns the bits of ``eigh``; beyond that a blocked Jacobi method works
        from global memory and sweeps counts its outer sweeps."""
        return self.eigh(a, vectors, _entry="ti_obs_eigh_wide", _max_n=_lib.EIGH_WIDE_MAX_N)

    def gedmd_spectrum_wide(self, gram, omega, a, nev, tol=0.0, vectors=True):
        """ti_obs_gedmd_spectrum_wide: ``gedmd_spectrum`` for p <= 1024 (p <= 64: the bits of ``gedmd_spectrum``)."""
        return self.gedmd_spectrum(gram, omega, a, nev, tol, vectors, _entry="ti_obs_gedmd_spectrum_wide")

    def gedmd_spectrum(self, gram, omega, a, nev, tol=0.0, vectors=True, _entry="ti_obs_gedmd_spectrum"):
        """ti_obs_gedmd_spectrum: (ev [.., nev] float64, vec [.., p, nev] complex128 or None, rank [..] int32) of a stack of Gram
        matrices [.., p, p], p <= 64 (numpy, or a CUDA complex128 tensor such as ``rff_gram`` returns: it stays on the GPU) and omega
        [d, p] float64 (host).  Lives where gram lives."""
        om = np.ascontiguousarray(omega, np.float64)
        if om.ndim != 2:
            raise ValueError(f"omega must be [d, p], got {om.shape}")
        d, p = om.shape
        gp, keep, dev, shape = self._complex_stack(gram, "gram")
        if len(shape) < 2 or tuple(shape[-2:]) != (p, p):
            raise ValueError(f"gram must be [.., {p}, {p}], got {tuple(shape)}")
        lead, nev = tuple(shape[:-2]), int(nev)
        n_mat = int(np.prod(lead, dtype=np.int64))
        like = keep if dev else None
        ev, ep = self._eig_out(like, (*lead, nev), "float64")
        vec, vp = self._eig_out(like, (*lead, p, nev, 2), "float64") if vectors else (None, None)
        rank, rp = self._eig_out(like, lead, "int32")
        desc = _lib.GedmdDesc(d, p, nev, 0, float(a), float(tol))
        _lib.check(getattr(_lib.lib(), _entry)(self.h, gp, n_mat, om.ctypes.data_as(C.POINTER(C.c_double)), C.byref(desc), ep, vp, rp,
                                               _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        if vec is not None:
            if dev:
                import torch
                vec = torch.view_as_complex(vec)
            else:
                vec = vec.view(np.complex128)[..., 0]
        return ev, vec, rank

    def weighted_histogram(self, values, logw, bins, range):
        """(hist [bins] float64, tails [3] float64 = weight below range[0], at or above range[1], of non-finite values).  values: a
        1-D float32 array or a column view such as cv[:, k] (read in place through its stride); logw None: uniform weights."""
        from . import observables as _obs
        bins, lo, hi = _obs.check_bins(bins, range)
        if len(values.shape) != 1:
            raise ValueError("values must be 1-D (a column of a CV array is fine: cv[:, k])")
        B = int(values.shape[0])
        if hasattr(values, "data_ptr"):
            if str(values.dtype) != "torch.float32":
                raise TypeError(f"values must be float32, got {values.dtype}")
            stride, vp, vdev, keep_v = int(values.stride(0)) if B > 1 else 1, C.c_void_p(values.data_ptr()), bool(values.is_cuda), values
        else:
            values = np.asarray(values)
            if values.dtype != np.float32:
                values = np.ascontiguousarray(values, np.float32)
            stride, vp, vdev, keep_v = (values.strides[0] // 4 if B > 1 else 1), C.c_void_p(values.ctypes.data), False, values
        if stride < 1:
            raise ValueError("values must have a positive stride")
        (lp,), ldev, keep = self._ptrs((logw, (B,), False, "logw"))
        if logw is not None and ldev != vdev:
            raise ValueError("values and logw must live in the same memory space")
        if vdev and logw is None:
            import torch
            self.wait_stream(torch.cuda.current_stream(self.device).cuda_stream)
        hist, tails = np.zeros(bins, np.float64), np.zeros(3, np.float64)
        dptr = C.POINTER(C.c_double)
        _lib.check(_lib.lib().ti_obs_hist(self.h, vp, stride, lp, B, bins, lo, hi, hist.ctypes.data_as(dptr), tails.ctypes.data_as(dptr),
                                          _lib.MEM_DEVICE if vdev else _lib.MEM_HOST))
        return hist, tails

    def _u8_in(self, a, B, what, dev):
        """(pointer, keepalive) of a [B] uint8 input living where the call lives (dev: on this engine's GPU)"""
        if dev:
            if not (hasattr(a, "data_ptr") and a.is_cuda and str(a.dtype) in ("torch.uint8", "torch.bool") and a.is_contiguous()):
                raise TypeError(f"{what} must be a contiguous CUDA uint8 (or bool) tensor when the call's buffers live on the GPU")
            if (a.device.index or 0) != self.device:
                raise ValueError(f"{what} lives on {a.device} but this engine was created on device {self.device}")
            if tuple(a.shape) != (B,):
                raise ValueError(f"{what} must have shape ({B},), got {tuple(a.shape)}")
            return C.c_void_p(a.data_ptr()), a
        host = np.ascontiguousarray(np.asarray(a.detach().cpu().numpy() if hasattr(a, "data_ptr") else a) != 0, np.uint8)
        if host.shape != (B,):
            raise ValueError(f"{what} must have shape ({B},), got {host.shape}")
        return C.c_void_p(host.ctypes.data), host

    def hist_cols(self, values, logw, keep, bins, lo, hi):
        """ti_obs_hist_cols: (hist [K, bins], tails [K, 3]) float64 of all K columns of values [B, K] float32 (contiguous; numpy or a
        CUDA tensor) in one launch, column c on [lo[c], hi[c]); logw [B] float32 (None: uniform) and keep [B] uint8 (None: all) live
        where values lives.  With keep the weights are normalised over the kept entries only."""
        from . import observables as _obs
        if len(values.shape) != 2 or int(values.shape[0]) < 1:
            raise ValueError("values must be [B, K] and non-empty")
        B, K = int(values.shape[0]), int(values.shape[1])
        if not 1 <= K <= _lib.HIST_COLS_MAX:
            raise ValueError(f"values must have 1..{_lib.HIST_COLS_MAX} columns, got {K}")
        lo, hi = np.ascontiguousarray(lo, np.float64).reshape(-1), np.ascontiguousarray(hi, np.float64).reshape(-1)
        if lo.shape != (K,) or hi.shape != (K,):
            raise ValueError(f"lo and hi must have K = {K} entries")
        for c in range(K):
            bins = _obs.check_bins(bins, (lo[c], hi[c]))[0]
        (vp, lp), dev, keep_alive = self._ptrs((values, (B, K), False, "values"), (logw, (B,), False, "logw"))
        kp, kk = (None, None) if keep is None else self._u8_in(keep, B, "keep", dev)
        hist, tails = np.zeros((K, bins), np.float64), np.zeros((K, 3), np.float64)
        dptr = C.POINTER(C.c_double)
        _lib.check(_lib.lib().ti_obs_hist_cols(self.h, vp, K, lp, kp, B, bins, lo.ctypes.data_as(dptr), hi.ctypes.data_as(dptr),
                                               hist.ctypes.data_as(dptr), tails.ctypes.data_as(dptr), _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        return hist, tails

    def _tica_values(self, values, what="values"):
        """(pointer, keepalive, is_device, n, K, stride, cstride) of values [n, K] float32 read in place through its strides: numpy,
        or a CUDA tensor -- a view such as z[:, 2:, 2] of a Z-matrix array is fine, its strides must be positive."""
        if len(values.shape) != 2 or int(values.shape[0]) < 1 or not 1 <= int(values.shape[1]) <= _lib.TICA_MAX_K:
            raise ValueError(f"{what} must be [n >= 1, 1 <= K <= {_lib.TICA_MAX_K}], got {tuple(values.shape)}")
        n, K = int(values.shape[0]), int(values.shape[1])
        if hasattr(values, "data_ptr") and values.is_cuda:
            if str(values.dtype) != "torch.float32":
                raise TypeError(f"{what} must be float32, got {values.dtype}")
            if (values.device.index or 0) != self.device:
                raise ValueError(f"{what} live on {values.device} but this engine was created on device {self.device}")
            cs = int(values.stride(1)) if K > 1 else 1
            s = int(values.stride(0)) if n > 1 else (K - 1) * cs + 1
            import torch
            self.wait_stream(torch.cuda.current_stream(self.device).cuda_stream)
            ptr, keep, dev = C.c_void_p(values.data_ptr()), values, True
        else:
            host = np.asarray(values.detach().cpu().numpy() if hasattr(values, "data_ptr") else values)
            if host.dtype != np.float32:
                host = np.ascontiguousarray(host, np.float32)
            cs = host.strides[1] // 4 if K > 1 else 1
            s = host.strides[0] // 4 if n > 1 else (K - 1) * cs + 1
            ptr, keep, dev = C.c_void_p(host.ctypes.data), host, False
        if cs < 1 or s < (K - 1) * cs + 1:
            raise ValueError(f"{what} must have positive strides with rows that do not overlap")
        return ptr, keep, dev, n, K, s, cs

    def _typed_in(self, a, shape, dtype, dev, what):
        """(pointer, keepalive) of an input of the given shape and dtype name living where the call lives"""
        if dev:
            if not (hasattr(a, "data_ptr") and a.is_cuda and str(a.dtype) == "torch." + dtype and a.is_contiguous()):
                raise TypeError(f"{what} must be a contiguous CUDA {dtype} tensor when the call's buffers live on the GPU")
            if (a.device.index or 0) != self.device:
                raise ValueError(f"{what} lives on {a.device} but this engine was created on device {self.device}")
            keep, ptr = a, C.c_void_p(a.data_ptr())
        else:
            keep = np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "data_ptr") else a, getattr(np, dtype))
            ptr = C.c_void_p(keep.ctypes.data)
        if tuple(keep.shape) != tuple(shape):
            raise ValueError(f"{what} must have shape {tuple(shape)}, got {tuple(keep.shape)}")
        return ptr, keep

    def tica_moments(self, values, traj_offsets, lags, encode=True):
        """ti_obs_tica_moments: (count [n_lag] int64, sum [n_lag, 2, d] float64, cov [n_lag, 3, d, d] float64) of the lagged pairs of
        values [n, K] float32 (numpy or a CUDA tensor, read in place through its strides) over the trajectories traj_offsets
        [n_traj + 1] at the lags [n_lag] (both host).  encode: d = 2 K, (cos, sin) of every value; else d = K.  cov holds (Sxx, Syy, Sxy).
        Lives where values lives."""
        vp, keep, dev, n, K, s, cs = self._tica_values(values)
        off = np.ascontiguousarray(traj_offsets, np.int64).reshape(-1)
        lg = np.ascontiguousarray(lags, np.int32).reshape(-1)
        if off.size < 2:
            raise ValueError("traj_offsets must have n_traj + 1 >= 2 entries")
        if not 1 <= lg.size <= _lib.TICA_MAX_LAGS:
            raise ValueError(f"lags must have 1..{_lib.TICA_MAX_LAGS} entries, got {lg.size}")
        d, L = (2 * K if encode else K), int(lg.size)
        like = keep if dev else None
        count, cp = self._eig_out(like, (L,), "int64")
        sm, sp = self._eig_out(like, (L, 2, d), "float64")
        cov, vp2 = self._eig_out(like, (L, 3, d, d), "float64")
        _lib.check(_lib.lib().ti_obs_tica_moments(self.h, vp, s, cs, n, K, int(bool(encode)), off.ctypes.data_as(C.POINTER(C.c_int64)), off.size - 1,
                                                  _lib.iptr(lg), L, cp, sp, vp2, _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        return count, sm, cov

    def tica_fit(self, count, sum, cov, dim=2, epsilon=1e-6, scaling=1):
        """ti_obs_tica_fit: (mean [n_lag, d], eigenvalues [n_lag, dim], components [n_lag, d, dim] float64, rank [n_lag] int32) of the
        moments ``tica_moments`` returns (numpy, or CUDA tensors: they stay on the GPU).  scaling 1: kinetic map, 0: none."""
        dev = hasattr(cov, "data_ptr") and cov.is_cuda
        if len(cov.shape) != 4 or int(cov.shape[1]) != 3 or int(cov.shape[2]) != int(cov.shape[3]):
            raise ValueError(f"cov must be [n_lag, 3, d, d], got {tuple(cov.shape)}")
        L, d, dim = int(cov.shape[0]), int(cov.shape[2]), int(dim)
        if dev:
            import torch
            self.wait_stream(torch.cuda.current_stream(self.device).cuda_stream)
        cp, k0 = self._typed_in(count, (L,), "int64", dev, "count")
        sp, k1 = self._typed_in(sum, (L, 2, d), "float64", dev, "sum")
        vp, k2 = self._typed_in(cov, (L, 3, d, d), "float64", dev, "cov")
        like = k2 if dev else None
        mean, mp = self._eig_out(like, (L, d), "float64")
        ev, ep = self._eig_out(like, (L, max(dim, 0)), "float64")
        comp, op = self._eig_out(like, (L, d, max(dim, 0)), "float64")
        rank, rp = self._eig_out(like, (L,), "int32")
        desc = _lib.TicaDesc(dim, int(scaling), 0, float(epsilon))
        _lib.check(_lib.lib().ti_obs_tica_fit(self.h, cp, sp, vp, L, d, C.byref(desc), mp, ep, op, rp, _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        return mean, ev, comp, rank

    def tica_transform(self, values, mean, comp, encode=True):
        """ti_obs_tica_transform: out [n_lag, B, dim] float32 = the projections of values [B, K] (as in ``tica_moments``) onto the
        components comp [n_lag, d, dim] about mean [n_lag, d] (float64, living where values lives)."""
        vp, keep, dev, B, K, s, cs = self._tica_values(values)
        if len(comp.shape) != 3:
            raise ValueError(f"comp must be [n_lag, d, dim], got {tuple(comp.shape)}")
        L, d, dim = (int(v) for v in comp.shape)
        if d != (2 * K if encode else K):
            raise ValueError(f"comp has d = {d} features but values has K = {K} columns (encode = {bool(encode)})")
        mp, k0 = self._typed_in(mean, (L, d), "float64", dev, "mean")
        cp, k1 = self._typed_in(comp, (L, d, dim), "float64", dev, "comp")
        out, op = self._eig_out(keep if dev else None, (L, B, dim), "float32")
        _lib.check(_lib.lib().ti_obs_tica_transform(self.h, vp, s, cs, B, K, int(bool(encode)), mp, cp, L, d, dim, op,
                                                    _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        return out

    def set_observer(self, descriptors, ref=None, select=None, every=1, out=None):
        """Attach an observer: every rollout that follows also writes the CVs of the grid points i % every == 0 and of the last one
        to out [rows, B, K] (float32 numpy array or CUDA tensor, rows = ti_rollout_rows(n_step, every); kept alive here).
        descriptors None detaches."""
        if descriptors is None:
            _lib.check(_lib.lib().ti_obs_set_observer(self.h, None, 0, None, None, 0, None, _lib.MEM_HOST))
            self._observer_keep = None
            return
        desc, r, sel, (dp, K, rp, sp) = self._obs_args(descriptors, ref, select)
        if out is None or len(out.shape) != 3 or int(out.shape[2]) != K:
            raise ValueError(f"out must be [rows, B, {K}]")
        (op,), dev, keep = self._ptrs((out, tuple(out.shape), True, "out"))
        _lib.check(_lib.lib().ti_obs_set_observer(self.h, dp, K, rp, sp, int(every), op, _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        self._observer_keep = out

    def _f64_in(self, a, B, what, dev):
        """(pointer, keepalive) of a [B] float64 input living where the call lives (dev: on this engine's GPU)"""
        if dev:
            if not (hasattr(a, "data_ptr") and a.is_cuda and str(a.dtype) == "torch.float64" and a.is_contiguous()):
                raise TypeError(f"{what} must be a contiguous CUDA float64 tensor when the call's buffers live on the GPU")
            if (a.device.index or 0) != self.device:
                raise ValueError(f"{what} lives on {a.device} but this engine was created on device {self.device}")
            if tuple(a.shape) != (B,):
                raise ValueError(f"{what} must have shape ({B},), got {tuple(a.shape)}")
            return C.c_void_p(a.data_ptr()), a
        host = np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "data_ptr") else a, np.float64)
        if host.shape != (B,):
            raise ValueError(f"{what} must have shape ({B},), got {host.shape}")
        return C.c_void_p(host.ctypes.data), host

    def ti_logw(self, u0, u1, neg_dlogp):
        """ti_obs_ti_logw: logw [B] float32 = -(u1 - u0 + neg_dlogp), formed in fp64 on the GPU and rounded once.  u0, u1 [B] float64
        (u0 None: 0), neg_dlogp [B] float32 (None: 0); numpy in, numpy out; CUDA tensors in, a CUDA tensor out."""
        B = int(u1.shape[0])
        dev = hasattr(u1, "data_ptr") and u1.is_cuda
        if dev:
            import torch
            out = torch.empty(B, dtype=torch.float32, device=u1.device)
        else:
            out = np.empty(B, np.float32)
        (np_, op), ndev, keep = self._ptrs((neg_dlogp, (B,), False, "neg_dlogp"), (out, (B,), True, "out"))
        if ndev != dev:
            raise ValueError("all buffers of a call must live in the same memory space (all host or all on the GPU)")
        p1, k1 = self._f64_in(u1, B, "u1", dev)
        p0, k0 = (None, None) if u0 is None else self._f64_in(u0, B, "u0", dev)
        _lib.check(_lib.lib().ti_obs_ti_logw(self.h, p0, p1, np_, B, op, _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        return out

    def bg_logw(self, z, u1=None, neg_dlogp_bg=None, neg_dlogp_ti=None, logpz=False):
        """ti_obs_bg_logw: logw [B] float32 = -(u1 + log N(z; 0, I) + neg_dlogp_bg + neg_dlogp_ti), formed in fp64 on the GPU and
        rounded once (the log of the reference's calc_importance_weights).  z [B, ...] float32, flattened per row; u1 [B] float64
        (None: 0); neg_dlogp_bg, neg_dlogp_ti [B] float32 (None: 0).  logpz=True: (logw, log N(z; 0, I) [B] float64).  numpy in,
        numpy out; CUDA tensors in, CUDA tensors out."""
        if len(z.shape) < 1 or int(z.shape[0]) < 1:
            raise ValueError("z must be [B, ...] and non-empty")
        B = int(z.shape[0])
        m = int(np.prod(z.shape[1:], dtype=np.int64))
        if not 1 <= m <= _lib.BG_MAX_M:
            raise ValueError(f"z must hold 1..{_lib.BG_MAX_M} components per row, got {m}")
        dev = hasattr(z, "data_ptr") and z.is_cuda
        if hasattr(z, "data_ptr"):
            if str(z.dtype) != "torch.float32" or not z.is_contiguous():
                raise TypeError("z must be a contiguous float32 tensor")
            z2 = z.reshape(B, m)
        else:
            z2 = np.ascontiguousarray(z, np.float32).reshape(B, m)
        if dev:
            import torch
            out = torch.empty(B, dtype=torch.float32, device=z.device)
            lp = torch.empty(B, dtype=torch.float64, device=z.device) if logpz else None
        else:
            out = np.empty(B, np.float32)
            lp = np.empty(B, np.float64) if logpz else None
        (zp, bp, tp, op), adev, keep = self._ptrs((z2, (B, m), False, "z"), (neg_dlogp_bg, (B,), False, "neg_dlogp_bg"),
                                                  (neg_dlogp_ti, (B,), False, "neg_dlogp_ti"), (out, (B,), True, "out"))
        if adev != dev:
            raise ValueError("all buffers of a call must live in the same memory space (all host or all on the GPU)")
        p1, k1 = (None, None) if u1 is None else self._f64_in(u1, B, "u1", dev)
        lpp = None if lp is None else C.c_void_p(lp.data_ptr() if dev else lp.ctypes.data)
        _lib.check(_lib.lib().ti_obs_bg_logw(self.h, zp, B, m, p1, bp, tp, lpp, op, _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        return (out, lp) if logpz else out

    def bg_ess(self, logpz, u1=None, neg_dlogp_bg=None, neg_dlogp_ti=None, keep=None):
        """ti_obs_bg_ess: (ess, kept) -- calc_ESS of the weights exp(-(u1 + logpz + neg_dlogp_bg + neg_dlogp_ti)) from their unrounded
        fp64 logarithms, over the molecules keep [B] marks (None: all).  logpz [B] float64 as ``bg_logw(..., logpz=True)`` returns
        it; the other arrays as in ``bg_logw``; all where logpz lives."""
        B = int(logpz.shape[0])
        dev = hasattr(logpz, "data_ptr") and logpz.is_cuda
        (bp, tp), adev, keepalive = self._ptrs((neg_dlogp_bg, (B,), False, "neg_dlogp_bg"), (neg_dlogp_ti, (B,), False, "neg_dlogp_ti"))
        if (neg_dlogp_bg is not None or neg_dlogp_ti is not None) and adev != dev:
            raise ValueError("all buffers of a call must live in the same memory space (all host or all on the GPU)")
        if dev and neg_dlogp_bg is None and neg_dlogp_ti is None:
            import torch
            self.wait_stream(torch.cuda.current_stream(self.device).cuda_stream)
        lp, k0 = self._f64_in(logpz, B, "logpz", dev)
        p1, k1 = (None, None) if u1 is None else self._f64_in(u1, B, "u1", dev)
        kp, k2 = (None, None) if keep is None else self._u8_in(keep, B, "keep", dev)
        ess, kept = C.c_double(0.0), C.c_int64(0)
        _lib.check(_lib.lib().ti_obs_bg_ess(self.h, lp, B, p1, bp, tp, kp, C.byref(ess), C.byref(kept), _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        return ess.value, kept.value

    # ---- velocity loss (ti_painn_vloss / ti_adw_vloss): the shared part of PainnEngine.velocity_loss and AdwEngine.velocity_loss
    @staticmethod
    def _vloss_desc(kind, gamma, a, center, t, t_distr, seed, traj_offset, draw, tbins):
        for name, table, value in (("kind", _lib.VLOSS_KINDS, kind), ("gamma", _lib.VLOSS_GAMMAS, gamma), ("center", _lib.VLOSS_CENTERS, center),
                                   ("t_distr", _lib.VLOSS_TDISTS, t_distr)):
            if value not in table:
                raise ValueError(f"{name} must be one of {sorted(table)}, got {value!r}")
        td = _lib.VLOSS_TDISTS["given" if t is not None else t_distr]
        if t is None and t_distr == "given":
            raise ValueError("t_distr='given' needs t")
        return _lib.VlossDesc(_lib.VLOSS_KINDS[kind], _lib.VLOSS_GAMMAS[gamma], float(a), _lib.VLOSS_CENTERS[center], td, int(seed),
                              int(traj_offset), int(draw), int(tbins))

    def _vloss(self, interp_only, xs, x0, x1, conds, desc, t, z, returns):
        """xs: the state shape [B, ...]; conds: buffer specs of the conditioning.  -> dict(loss [B] float64, mean, tbins [n, 2] |
        None, rows = the divisor of mean, and the entries of `returns` among t [B], z, xt [2, ...], b [2, ...]); arrays live where x0 lives."""
        B = int(xs[0])
        bad = set(returns) - ({"t", "z", "xt"} if interp_only else {"t", "z", "xt", "b"})
        if bad:
            raise ValueError(f"unknown entries in returns: {sorted(bad)}")
        dev_like = x0 if hasattr(x0, "data_ptr") and x0.is_cuda else None
        two = desc.kind == _lib.VLOSS_KINDS["standard"]
        res = {}
        if "t" in returns or interp_only:
            res["t"] = _alloc_like(dev_like, (B,))
        if ("z" in returns or interp_only) and two:
            res["z"] = _alloc_like(dev_like, xs)
        if "xt" in returns or interp_only:
            res["xt"] = _alloc_like(dev_like, (2,) + tuple(xs))
        if "b" in returns:
            res["b"] = _alloc_like(dev_like, (2,) + tuple(xs))
        specs = [(x0, xs, False, "x0"), (x1, xs, False, "x1"), *conds, (t, (B,), False, "t"), (z, xs, False, "z"),
                 (res.get("t"), (B,), True, "out_t"), (res.get("z"), xs, True, "out_z"), (res.get("xt"), None, True, "out_xt"),
                 (res.get("b"), None, True, "out_b")]
        ptrs, dev, keep = self._ptrs(*specs)
        x0p, x1p, *cp = ptrs[:2 + len(conds)]
        tp, zp, otp, ozp, oxp, obp = ptrs[2 + len(conds):]
        mem = _lib.MEM_DEVICE if dev else _lib.MEM_HOST
        L = _lib.lib()
        painn = isinstance(self, PainnEngine)
        if interp_only:
            fn = L.ti_painn_vloss_interp if painn else L.ti_adw_vloss_interp
            _lib.check(fn(self.h, C.byref(desc), x0p, x1p, tp, zp, B, otp, ozp, oxp, mem))
        else:
            if dev:
                import torch
                loss = torch.empty(B, dtype=torch.float64, device=x0.device)
                lp = C.c_void_p(loss.data_ptr())
            else:
                loss = np.empty(B, np.float64)
                lp = C.c_void_p(loss.ctypes.data)
            mean = C.c_double(0.0)
            tb = np.zeros((desc.n_tbins, 2), np.float64) if desc.n_tbins > 0 else None
            tbp = tb.ctypes.data_as(C.POINTER(C.c_double)) if tb is not None else None
            fn = L.ti_painn_vloss if painn else L.ti_adw_vloss
            _lib.check(fn(self.h, C.byref(desc), x0p, x1p, *cp, tp, zp, B, lp, C.byref(mean), tbp, otp, ozp, oxp, obp, mem))
            res.update(loss=loss, mean=mean.value, tbins=tb, rows=B * (self.A if painn else 1))
        if not two:                                   # the one-sided loss has no minus half
            for k in ("xt", "b"):
                if k in res:
                    res[k] = res[k][:1]
        return res

    def _times(self, t, B):
        """A 1-D time vector of length B (one time per molecule / row) as a buffer spec, or None for a scalar t."""
        if (tuple(t.shape) if hasattr(t, "shape") else np.shape(t)) == ():
            return None
        if len(t.shape) != 1 or int(t.shape[0]) != B:
            raise ValueError(f"t must be a scalar or a 1-D array of length B = {B}")
        return (t, (B,), False, "t")


class PainnEngine(_Engine):
    """cPaiNN drift + fixed-step integrator for one molecular species (homogeneous batches)."""

    def __init__(self, variant, F, L, A, edge_src, edge_dst, edge_type, atom_ids, flat_weights, *, n_types=25, temp_length=10.0,
                 time_length=10.0, length_scale=10.0, temperatures=(300, 400, 500, 600, 700, 800, 900, 1000), device=0, precision="f32"):
        if precision not in _lib.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_lib.PRECISIONS)}")
        self.precision = precision
        temps = np.asarray(temperatures, np.float32)
        es, ed, et, ai = (np.ascontiguousarray(a, np.int32) for a in (edge_src, edge_dst, edge_type, atom_ids))
        if not (es.shape == ed.shape == et.shape) or es.ndim != 1 or ai.shape != (A,):
            raise ValueError("edge_src/edge_dst/edge_type must be 1-D and equally long; atom_ids must have A entries")
        self.variant, self.F, self.L, self.A, self.E = int(variant), int(F), int(L), int(A), int(es.size)
        self.ncond = W.N_COND[self.variant]
        self.desc = _lib.PainnDesc(self.variant, self.F, self.L, int(n_types), self.A, self.E, float(temp_length), float(time_length),
                                   float(length_scale), float(temps.mean(dtype=np.float32)), float(temps.max() - temps.min()), _lib.PRECISIONS[precision])
        w = np.ascontiguousarray(flat_weights, np.float32)
        self.device = int(device)
        self.h = _lib.lib().ti_painn_create(C.byref(self.desc), _lib.fptr(w), w.size, _lib.iptr(es), _lib.iptr(ed), _lib.iptr(et),
                                            _lib.iptr(ai), self.device)
        if not self.h:
            raise _lib.TiError(-1, _lib.last_error())

    TEMPLATES = {"auto": -1, "throughput": 0, "latency": 1, "pair": 2}

    def set_template(self, which: str = "auto"):
        """Pin the edge-row layout ('throughput' | 'latency': directed rows; 'pair': pair-major rows, the filter branch once per atom
        pair -- falls back to 'throughput' where no pair layout exists) or let each call choose from its batch size ('auto')."""
        _lib.check(_lib.lib().ti_painn_set_template(self.h, self.TEMPLATES[which]))

    def template_for(self, B: int) -> str:
        """The layout a drift / rollout call over B molecules would use."""
        rc = _lib.lib().ti_painn_template_for(self.h, int(B))
        if rc < 0:
            _lib.check(rc)
        return {0: "throughput", 1: "latency", 2: "pair"}[rc]

    def set_edge_mask(self, mask):
        """Per-molecule edge sets over this engine's template: mask [B, A] uint32 (or int32, same bits), bit s of mask[b, d] set when
        the edge s -> d exists in molecule b; template edges whose bit is clear contribute nothing to molecule b.  It stays in force
        for every later call over B molecules (another B is refused) until set_edge_mask(None).  A numpy array is copied; a CUDA
        tensor is read on the device."""
        L = _lib.lib()
        if mask is None:
            _lib.check(L.ti_painn_set_edge_mask(self.h, None, 0, _lib.MEM_HOST))
            return
        if hasattr(mask, "data_ptr"):                                 # torch.Tensor without importing torch
            if str(mask.dtype) not in ("torch.int32", "torch.uint32"):
                raise TypeError(f"mask must be int32 or uint32, got {mask.dtype}")
            if len(mask.shape) != 2 or int(mask.shape[1]) != self.A:
                raise ValueError(f"mask must be [B,{self.A}], got {tuple(mask.shape)}")
            B = int(mask.shape[0])
            if mask.is_cuda:
                if mask.device.index != self.device:
                    raise ValueError(f"mask lives on cuda:{mask.device.index} but this engine was created on device {self.device}")
                mask = mask.contiguous()
                import torch
                torch.cuda.current_stream(self.device).synchronize()
                _lib.check(L.ti_painn_set_edge_mask(self.h, C.c_void_p(mask.data_ptr()), B, _lib.MEM_DEVICE))
                return
            mask = mask.numpy()
        m = np.asarray(mask)
        if m.dtype not in (np.uint32, np.int32):
            raise TypeError(f"mask must be uint32 or int32, got {m.dtype}")
        if m.ndim != 2 or m.shape[1] != self.A:
            raise ValueError(f"mask must be [B,{self.A}], got {m.shape}")
        m = np.ascontiguousarray(m.view(np.uint32))
        _lib.check(L.ti_painn_set_edge_mask(self.h, C.c_void_p(m.ctypes.data), int(m.shape[0]), _lib.MEM_HOST))

    def set_molecules(self, n_atoms, mask=None, pair_type=None):
        """Mixed-species batches over this engine's template (A = the largest molecule): n_atoms [B] in 1..A -- atoms a >= n_atoms[b]
        of molecule b are pad atoms (drift exactly 0, never moved, no noise; what they carry never reaches a real atom); mask [B, A]
        as in set_edge_mask (None: every template edge between real atoms); pair_type [B, A, A] in 0..3, the type of the edge s -> d
        of molecule b at [b, s, d] (None: the template's types).  Replaces an edge mask in force and is replaced by set_edge_mask;
        set_molecules(None) clears it.  Host arrays (numpy, or CPU tensors) are copied."""
        L = _lib.lib()
        if n_atoms is None:
            _lib.check(L.ti_painn_set_molecules(self.h, None, None, None, 0, _lib.MEM_HOST))
            return
        host = lambda a: a.detach().cpu().numpy() if hasattr(a, "data_ptr") else np.asarray(a)
        n = np.ascontiguousarray(host(n_atoms), np.int32)
        if n.ndim != 1 or n.size < 1:
            raise ValueError("n_atoms must be a non-empty 1-D array")
        B = int(n.size)
        m = t = None
        if mask is not None:
            m = host(mask)
            if m.dtype not in (np.uint32, np.int32):
                raise TypeError(f"mask must be uint32 or int32, got {m.dtype}")
            if m.shape != (B, self.A):
                raise ValueError(f"mask must be [{B},{self.A}], got {m.shape}")
            m = np.ascontiguousarray(m.view(np.uint32))
        if pair_type is not None:
            t = host(pair_type)
            if t.shape != (B, self.A, self.A):
                raise ValueError(f"pair_type must be [{B},{self.A},{self.A}], got {t.shape}")
            if t.size and (t.min() < 0 or t.max() > 3):
                raise ValueError("pair_type entries must be in 0..3")
            t = np.ascontiguousarray(t, np.uint8)
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        _lib.check(L.ti_painn_set_molecules(self.h, ptr(n), ptr(m), ptr(t), B, _lib.MEM_HOST))

    def set_forcefield(self, ff):
        """ti_obs_ff_set: copy a forcefield.ForceField of this engine's species into the handle (None clears it).  The library checks
        index ranges, repeated atoms, the caps, signs and finiteness; the dense pair table is built here (ForceField.pair_table).  The
        masses are uploaded when the force field has them (ti_obs_ff_set_masses)."""
        L = _lib.lib()
        self._ff_set, self._ff_constraints, self._ff_masses = False, False, False
        if ff is None:
            _lib.check(L.ti_obs_ff_set(self.h, None, None, None, None, None, None, None, None))
            return
        pairs = ff.pair_table(self.A)
        desc = _lib.FfDesc(len(ff.bond_idx), len(ff.angle_idx), len(ff.torsion_idx), len(pairs), float(ff.coulomb))
        ip = lambda a: _lib.iptr(a) if a.size else None
        dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a.size else None
        _lib.check(L.ti_obs_ff_set(self.h, C.byref(desc), ip(ff.bond_idx), dp(ff.bond_par), ip(ff.angle_idx), dp(ff.angle_par),
                                   ip(ff.torsion_idx), dp(ff.torsion_par), dp(pairs)))
        self._ff_set, self._ff_constraints = True, bool(getattr(ff, "has_constraints", False))
        m = getattr(ff, "masses", None)                           # for langevin only, which refuses a missing or zero mass itself
        if m is not None and len(m) == self.A and np.isfinite(m).all() and (np.asarray(m) > 0).all():
            m = np.ascontiguousarray(m, np.float64)
            _lib.check(L.ti_obs_ff_set_masses(self.h, dp(m)))
            self._ff_masses = True

    def ff_energy(self, x, to_nm=1.0, T=None, terms=False):
        """ti_obs_ff_energy: E [B] float64 of x [B,A,3] float32 at positions x * to_nm (nm), in kJ/mol -- or, with T [B] float32 kelvin
        (a scalar: every molecule's), the reduced energy E / (R T).  terms=True: (E, terms [B, 4]) with the bond, angle, torsion and
        pair sums.  numpy in, numpy out; a CUDA tensor in, CUDA float64 tensors out (no coordinate-sized host copy)."""
        B = self._check_x(x)
        dev = hasattr(x, "data_ptr") and x.is_cuda
        if T is not None and (np.shape(T) if not hasattr(T, "shape") else tuple(T.shape)) == ():
            T = x.new_full((B,), float(T)) if dev else np.full(B, float(T), np.float32)
        elif T is not None and not dev and not hasattr(T, "data_ptr"):
            T = np.ascontiguousarray(T, np.float32)
        if dev:
            import torch
            e = torch.empty(B, dtype=torch.float64, device=x.device)
            tm = torch.empty((B, 4), dtype=torch.float64, device=x.device) if terms else None
            ep, tp2 = C.c_void_p(e.data_ptr()), (C.c_void_p(tm.data_ptr()) if terms else None)
        else:
            e, tm = np.empty(B, np.float64), (np.empty((B, 4), np.float64) if terms else None)
            ep, tp2 = C.c_void_p(e.ctypes.data), (C.c_void_p(tm.ctypes.data) if terms else None)
        (xp, Tp), xdev, keep = self._ptrs((x, (B, self.A, 3), False, "x"), (T, (B,), False, "T"))
        _lib.check(_lib.lib().ti_obs_ff_energy(self.h, xp, B, float(to_nm), Tp, ep, tp2, _lib.MEM_DEVICE if xdev else _lib.MEM_HOST))
        return (e, tm) if terms else e

    def ff_forces(self, x, to_nm=1.0, T=None, energy=False):
        """ti_obs_ff_forces: F [B,A,3] float64 = -dE / d(position in nm) of x [B,A,3] float32 at positions x * to_nm, in kJ / (mol nm)
        -- or, with T [B] float32 kelvin (a scalar: every molecule's), divided by R T.  energy=True: (F, E [B]) with the energy of the
        same pass.  numpy in, numpy out; a CUDA tensor in, CUDA float64 tensors out."""
        B = self._check_x(x)
        dev = hasattr(x, "data_ptr") and x.is_cuda
        if T is not None and (np.shape(T) if not hasattr(T, "shape") else tuple(T.shape)) == ():
            T = x.new_full((B,), float(T)) if dev else np.full(B, float(T), np.float32)
        elif T is not None and not dev and not hasattr(T, "data_ptr"):
            T = np.ascontiguousarray(T, np.float32)
        if dev:
            import torch
            f = torch.empty((B, self.A, 3), dtype=torch.float64, device=x.device)
            e = torch.empty(B, dtype=torch.float64, device=x.device) if energy else None
            fp, ep = C.c_void_p(f.data_ptr()), (C.c_void_p(e.data_ptr()) if energy else None)
        else:
            f, e = np.empty((B, self.A, 3), np.float64), (np.empty(B, np.float64) if energy else None)
            fp, ep = C.c_void_p(f.ctypes.data), (C.c_void_p(e.ctypes.data) if energy else None)
        (xp, Tp), xdev, keep = self._ptrs((x, (B, self.A, 3), False, "x"), (T, (B,), False, "T"))
        _lib.check(_lib.lib().ti_obs_ff_forces(self.h, xp, B, float(to_nm), Tp, fp, ep, _lib.MEM_DEVICE if xdev else _lib.MEM_HOST))
        return (f, e) if energy else f

    def langevin(self, pos, vel, T, dt, friction, n_steps, stride=0, step_offset=0, traj_offset=0, seed=0, ids=None, to_nm=1.0,
                 draw_velocities=False, steps_per_launch=0, frames=True, energies=True):
        """ti_obs_ff_langevin: n_steps of OpenMM's Langevin "middle" scheme for the replicas pos [B,A,3] float64 (nm), vel [B,A,3]
        float64 (nm/ps; None with draw_velocities) at the temperatures T [B] kelvin (a scalar: every replica's) under the force field
        and masses set with set_forcefield; dt in ps, friction in 1/ps (0: NVE).  Returns (pos, vel, frames, epot, ekin): the new state
        (the inputs are not changed), frames [B, n_steps // stride, A, 3] float32 in model units nm / to_nm, centred, and the potential
        and kinetic energies [B, n_steps // stride] float64 at the frames (None where frames / energies is off or stride is 0).  numpy
        in, numpy out; CUDA tensors in, CUDA tensors out.  Raises ValueError for a force field with constraints (they are not
        integrated) and for missing masses."""
        return self._md(None, pos, vel, T, dt, friction, n_steps, stride, step_offset, traj_offset, seed, ids, to_nm, draw_velocities,
                        steps_per_launch, frames, energies)

    def remd(self, pos, vel, T, n_rungs, exchange_every, dt, friction, n_steps, stride=0, step_offset=0, traj_offset=0, seed=0, ids=None,
             ladder_ids=None, walker=None, to_nm=1.0, draw_velocities=False, steps_per_launch=0, frames=True, energies=True):
        """ti_obs_ff_remd: langevin with Metropolis exchanges of neighbouring rungs after every exchange_every-th global step.  The B
        rows are n_ladders ladders of n_rungs rungs, row l * n_rungs + k rung k of ladder l; T [B] is the temperature of each row and
        stays with the row, the configurations move.  ladder_ids [n_ladders] int64 key the exchange draws (None: 0, 1, ...); walker
        [B] int32 says at which rung the configuration now at a row started (None: the identity).  Returns (pos, vel, frames, epot,
        ekin, walker, walkers, counts): langevin's five, the labels after the call, after each of its attempts [n_attempts, B] and the
        attempts and acceptances of every neighbouring pair in this call [n_ladders, n_rungs - 1, 2] int64.  A frame due at the step of
        an attempt shows the state before the exchange.  numpy in, numpy out; CUDA tensors in, CUDA tensors out; langevin's
        ValueErrors."""
        return self._md((int(n_rungs), int(exchange_every), ladder_ids, walker), pos, vel, T, dt, friction, n_steps, stride, step_offset,
                        traj_offset, seed, ids, to_nm, draw_velocities, steps_per_launch, frames, energies)

    def _md(self, remd, pos, vel, T, dt, friction, n_steps, stride, step_offset, traj_offset, seed, ids, to_nm, draw_velocities,
            steps_per_launch, frames, energies):
        """langevin (remd None) or remd ((n_rungs, exchange_every, ladder_ids, walker)): the checks, the buffers and the call"""
        if not getattr(self, "_ff_set", False):
            raise ValueError("langevin needs a force field (set_forcefield)")
        if self._ff_constraints:
            raise ValueError("the force field lists constraints, which are not integrated: export the System without them (rigidWater=False, constraints=None)")
        if not self._ff_masses:
            raise ValueError("langevin needs a force field with masses, every one > 0 (ForceField.masses)")
        if pos is None or len(pos.shape) != 3 or tuple(pos.shape[1:]) != (self.A, 3):
            raise ValueError(f"pos must be [B,{self.A},3]")
        B = int(pos.shape[0])
        dev = hasattr(pos, "data_ptr") and pos.is_cuda
        if vel is None and not draw_velocities:
            raise ValueError("vel is None and draw_velocities is off")
        n_frames = int(n_steps) // int(stride) if stride and stride > 0 else 0
        if dev:
            import torch
            if pos.device.index != self.device:
                raise ValueError(f"pos lives on {pos.device} but this engine was created on device {self.device}")
            t64 = lambda a: a.detach().to(dtype=torch.float64, copy=True).contiguous()
            p = t64(pos)
            v = torch.empty_like(p) if draw_velocities else t64(vel)
            Td = torch.full((B,), float(T), dtype=torch.float32, device=pos.device) if not hasattr(T, "shape") or tuple(T.shape) == () \
                else torch.as_tensor(T, dtype=torch.float32, device=pos.device).contiguous()
            idd = None if ids is None else torch.as_tensor(ids, dtype=torch.int64, device=pos.device).contiguous()
            new = lambda shape, dt_: torch.empty(shape, dtype=dt_, device=pos.device)
            fr = new((B, n_frames, self.A, 3), torch.float32) if frames and n_frames else None
            ep = new((B, n_frames), torch.float64) if energies and n_frames else None
            ek = new((B, n_frames), torch.float64) if energies and n_frames else None
            ptr = lambda a: None if a is None else C.c_void_p(a.data_ptr())
            self.wait_stream(torch.cuda.current_stream(self.device).cuda_stream)      # behind the copies and fills above
        else:
            p = np.array(pos, np.float64, order="C")
            v = np.empty_like(p) if draw_velocities else np.array(vel, np.float64, order="C")
            Td = np.full(B, float(T), np.float32) if np.shape(T) == () else np.ascontiguousarray(T, np.float32)
            idd = None if ids is None else np.ascontiguousarray(ids, np.int64)
            fr = np.empty((B, n_frames, self.A, 3), np.float32) if frames and n_frames else None
            ep = np.empty((B, n_frames), np.float64) if energies and n_frames else None
            ek = np.empty((B, n_frames), np.float64) if energies and n_frames else None
            ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        if tuple(v.shape) != (B, self.A, 3) or tuple(Td.shape) != (B,) or (idd is not None and tuple(idd.shape) != (B,)):
            raise ValueError(f"vel must be [{B},{self.A},3], T and ids [{B}]")
        if fr is None and ep is None:                             # no frame is asked for or none falls into the call
            stride = 0
        desc = _lib.MdDesc(float(dt), float(friction), int(n_steps), int(stride), int(step_offset), int(traj_offset), int(seed),
                           int(bool(draw_velocities)), int(steps_per_launch))
        if remd is None:
            _lib.check(_lib.lib().ti_obs_ff_langevin(self.h, C.byref(desc), ptr(p), ptr(v), ptr(Td), ptr(idd), B, float(to_nm), ptr(fr), ptr(ep),
                                                     ptr(ek), _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
            return p, v, fr, ep, ek
        K, every, ladder_ids, walker = remd
        if K < 2 or B % K or every < 1:
            raise ValueError(f"n_rungs must be >= 2 and divide B = {B}, exchange_every must be >= 1")
        n_att = (int(step_offset) + int(n_steps)) // every - int(step_offset) // every
        if dev:
            lid = None if ladder_ids is None else torch.as_tensor(ladder_ids, dtype=torch.int64, device=pos.device).contiguous()
            wk = torch.arange(B, dtype=torch.int32, device=pos.device) % K if walker is None \
                else torch.as_tensor(walker, device=pos.device).to(dtype=torch.int32, copy=True).contiguous()
            hist, cnt = new((n_att, B), torch.int32), new((B // K, K - 1, 2), torch.int64)
            self.wait_stream(torch.cuda.current_stream(self.device).cuda_stream)
        else:
            lid = None if ladder_ids is None else np.ascontiguousarray(ladder_ids, np.int64)
            wk = (np.arange(B) % K).astype(np.int32) if walker is None else np.array(walker, np.int32, order="C")
            hist, cnt = np.empty((n_att, B), np.int32), np.empty((B // K, K - 1, 2), np.int64)
        if tuple(wk.shape) != (B,) or (lid is not None and tuple(lid.shape) != (B // K,)):
            raise ValueError(f"walker must be [{B}], ladder_ids [{B // K}]")
        rd = _lib.RemdDesc(K, 0, every)
        _lib.check(_lib.lib().ti_obs_ff_remd(self.h, C.byref(desc), C.byref(rd), ptr(p), ptr(v), ptr(Td), ptr(idd), ptr(lid), B, float(to_nm),
                                             ptr(wk), ptr(fr), ptr(ep), ptr(ek), ptr(hist) if n_att else None, ptr(cnt),
                                             _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        return p, v, fr, ep, ek, wk, hist, cnt

    def _zmat_topology(self, zm):
        if zm.A != self.A:
            raise ValueError(f"the Z-matrix is for A = {zm.A} atoms, this engine has A = {self.A}")
        return _lib.iptr(zm.order), _lib.iptr(zm.ref)

    def zmatrix(self, x, zm, out=None):
        """ti_obs_zmat: z [B, A-1, 3] float32 of x [B, A, 3] under the topology zm (zmatrix.ZMatrix): row s - 1 holds (d, a, t) of
        sorted atom s.  numpy in, numpy out; a CUDA tensor in, a CUDA tensor out."""
        op_, rp = self._zmat_topology(zm)
        B = self._check_x(x)
        if out is None:
            out = _alloc_like(x if hasattr(x, "data_ptr") and x.is_cuda else None, (B, self.A - 1, 3))
        (xp, zp), dev, keep = self._ptrs((x, (B, self.A, 3), False, "x"), (out, (B, self.A - 1, 3), True, "out"))
        _lib.check(_lib.lib().ti_obs_zmat(self.h, op_, rp, xp, B, zp, _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        return out

    def zmatrix_xyz(self, z, zm, logdet=False, valid=False):
        """ti_obs_zmat_xyz: x [B, A, 3] float32 of z [B, A-1, 3] in the caller's atom numbering (NeRF placement in the reference's
        canonical frame); logdet=True adds log|det J| [B] float64, valid=True the validity mask [B] uint8 (a tuple in that order).
        numpy in, numpy out; a CUDA tensor in, CUDA tensors out."""
        op_, rp = self._zmat_topology(zm)
        if z is None or len(z.shape) != 3 or tuple(z.shape[1:]) != (self.A - 1, 3):
            raise ValueError(f"z must be [B,{self.A - 1},3]")
        B = int(z.shape[0])
        dev_in = hasattr(z, "data_ptr") and z.is_cuda
        x = _alloc_like(z if dev_in else None, (B, self.A, 3))
        ld = vd = lp = vp = None
        if dev_in:
            import torch
            if logdet:
                ld = torch.empty(B, dtype=torch.float64, device=z.device); lp = C.c_void_p(ld.data_ptr())
            if valid:
                vd = torch.empty(B, dtype=torch.uint8, device=z.device); vp = C.c_void_p(vd.data_ptr())
        else:
            if logdet:
                ld = np.empty(B, np.float64); lp = C.c_void_p(ld.ctypes.data)
            if valid:
                vd = np.empty(B, np.uint8); vp = C.c_void_p(vd.ctypes.data)
        (zp, xp), dev, keep = self._ptrs((z, (B, self.A - 1, 3), False, "z"), (x, (B, self.A, 3), True, "out"))
        _lib.check(_lib.lib().ti_obs_zmat_xyz(self.h, op_, rp, zp, B, xp, lp, vp, _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        res = (x,) + ((ld,) if logdet else ()) + ((vd,) if valid else ())
        return res[0] if len(res) == 1 else res

    def _obs_x_shape(self, x):
        B = self._check_x(x)
        return B, (B, self.A, 3)

    def _check_x(self, x, name="x"):
        if x is None or len(x.shape) != 3 or tuple(x.shape[1:]) != (self.A, 3):
            raise ValueError(f"{name} must be [B,{self.A},3]")
        return int(x.shape[0])

    def _cond_spec(self, cond, B):
        if self.ncond and cond is None:
            raise ValueError("this variant needs per-node conditioning (cond)")
        return (cond if self.ncond else None, (B, self.A, self.ncond), False, "cond")

    def drift(self, x, t, cond=None, out=None):
        """x [B,A,3] -> drift [B,A,3] at time t: a scalar, or a 1-D array of B times (one per molecule)."""
        B = self._check_x(x)
        if out is None:
            out = _alloc_like(x if hasattr(x, "data_ptr") and x.is_cuda else None, (B, self.A, 3))
        tv = self._times(t, B)
        if tv is not None:
            (xp, tp, cp, op), dev, keep = self._ptrs((x, (B, self.A, 3), False, "x"), tv, self._cond_spec(cond, B), (out, (B, self.A, 3), True, "out"))
            _lib.check(_lib.lib().ti_painn_drift_tv(self.h, xp, tp, cp, B, op, _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
            return out
        (xp, cp, op), dev, keep = self._ptrs((x, (B, self.A, 3), False, "x"), self._cond_spec(cond, B), (out, (B, self.A, 3), True, "out"))
        _lib.check(_lib.lib().ti_painn_drift(self.h, xp, float(t), cp, B, op, _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        return out

    def velocity_loss(self, x0, x1, cond=None, *, kind="standard", gamma="brownian", a=1.0, center="batch", t=None, t_distr="uniform",
                      z=None, seed=0, traj_offset=0, draw=0, tbins=0, returns=()):
        """ti_painn_vloss: the stochastic-interpolant velocity loss of this model on the pairs (x0, x1) [B,A,3] -- the antithetic states
        of the interpolant (kind 'standard': (1 - t) x0 + t x1 +- gamma(t) z; 'one_sided': t x1 + (1 - t) x0 with x0 the noise), centred
        per 'batch' (the reference's mean over all atom rows of the call), per 'molecule' or not at all ('none'), the drift on both, and
        the per-molecule sums.  t [B] / z [B,A,3] given, or drawn from Philox by (seed, traj_offset + b, draw): t_distr 'uniform',
        'beta_half' (Beta(1/2, 1/2)) or 'beta_2_1' (Beta(2, 1)).  -> dict: loss [B] float64, mean (sum of loss / (B A)), tbins [n, 2]
        (sum, count per bin of t) or None, plus the entries named in returns: 't', 'z', 'xt' [2,B,A,3], 'b' [2,B,A,3] (one_sided: [1,...])."""
        B = self._check_x(x0, "x0")
        desc = self._vloss_desc(kind, gamma, a, center, t, t_distr, seed, traj_offset, draw, tbins)
        return self._vloss(False, (B, self.A, 3), x0, x1, [self._cond_spec(cond, B)], desc, t, z, returns)

    def interpolate(self, x0, x1, *, kind="standard", gamma="brownian", a=1.0, center="batch", t=None, t_distr="uniform", z=None, seed=0,
                    traj_offset=0, draw=0):
        """ti_painn_vloss_interp: stage one of velocity_loss alone -> dict: t [B], z [B,A,3] (standard), xt [2,B,A,3] (one_sided: [1,...])."""
        B = self._check_x(x0, "x0")
        desc = self._vloss_desc(kind, gamma, a, center, t, t_distr, seed, traj_offset, draw, 0)
        return self._vloss(True, (B, self.A, 3), x0, x1, [], desc, t, z, ())

    def rollout(self, x0, cond, t_grid, scheme="euler", save_every=1, eps=0.0, seed=0, traj_offset=0, com_free_noise=False, out=None,
                rtol=1e-4, atol=1e-4, step_offset=0, step_control="batch"):
        """Returns (path [rows,B,A,3], n_fevals).  scheme: 'euler' | 'heun' | 'em' | 'midpoint' | 'rk4' on the grid, or 'dopri5'
        (adaptive, tolerances rtol / atol; the grid then only selects the output times).  step_offset: EM noise counter of the
        call's first step (pass the number of steps already taken when continuing a trajectory).  step_control='trajectory' (dopri5
        only): every molecule gets its own step sizes -- the result a batch of one gives; n_fevals then counts batched evaluations
        and step_counts(B) returns the per-molecule accepted / rejected steps."""
        B = self._check_x(x0, "x0")
        on_gpu = hasattr(x0, "data_ptr") and x0.is_cuda
        rd = _rollout_desc(scheme, t_grid, save_every, _lib.MEM_DEVICE if on_gpu else _lib.MEM_HOST, eps, seed, traj_offset, com_free_noise,
                           rtol, atol, step_offset, step_control)
        rows = int(_lib.lib().ti_rollout_rows(rd.n_step, rd.save_every))
        if out is None:
            out = _alloc_like(x0 if on_gpu else None, (rows, B, self.A, 3))
        (xp, cp, op), dev, keep = self._ptrs((x0, (B, self.A, 3), False, "x0"), self._cond_spec(cond, B), (out, (rows, B, self.A, 3), True, "out"))
        nfe = C.c_int64(0)
        _lib.check(_lib.lib().ti_painn_rollout(self.h, C.byref(rd), xp, cp, B, op, C.byref(nfe)))
        return out, nfe.value

    # ---- forward-mode derivative, exact divergence, dlogp
    def jvp(self, x, xdot, t, cond=None):
        """(b(x), (d b / d x) xdot), both [B,A,3]."""
        B = self._check_x(x)
        like = x if hasattr(x, "data_ptr") and x.is_cuda else None
        out, tan = _alloc_like(like, (B, self.A, 3)), _alloc_like(like, (B, self.A, 3))
        (xp, tp, cp, op, tnp), dev, keep = self._ptrs((x, (B, self.A, 3), False, "x"), (xdot, (B, self.A, 3), False, "xdot"), self._cond_spec(cond, B),
                                                      (out, None, True, "out"), (tan, None, True, "out_tan"))
        _lib.check(_lib.lib().ti_painn_drift_jvp(self.h, xp, tp, float(t), cp, B, op, tnp, _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        return out, tan

    def drift_div(self, x, t, cond=None):
        """(b(x) [B,A,3], div [B]) with div = sum_ij d b_ij / d x_ij -- the reference's compute_divergence without its 1e-2.
        t: a scalar or one time per molecule ([B])."""
        B = self._check_x(x)
        like = x if hasattr(x, "data_ptr") and x.is_cuda else None
        out, div = _alloc_like(like, (B, self.A, 3)), _alloc_like(like, (B,))
        tv = self._times(t, B)
        if tv is not None:
            (xp, tp, cp, op, dp), dev, keep = self._ptrs((x, (B, self.A, 3), False, "x"), tv, self._cond_spec(cond, B), (out, None, True, "out"),
                                                         (div, None, True, "out_div"))
            _lib.check(_lib.lib().ti_painn_drift_div_tv(self.h, xp, tp, cp, B, op, dp, _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
            return out, div
        (xp, cp, op, dp), dev, keep = self._ptrs((x, (B, self.A, 3), False, "x"), self._cond_spec(cond, B), (out, None, True, "out"), (div, None, True, "out_div"))
        _lib.check(_lib.lib().ti_painn_drift_div(self.h, xp, float(t), cp, B, op, dp, _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        return out, div

    def rollout_dlogp(self, x0, cond, t_grid, scheme="euler", save_every=1, div_scale=1.0, out_scale=1.0, reverse_ode=False,
                      rtol=1e-4, atol=1e-4, step_control="batch"):
        """Two-state rollout (x, dlogp): returns (path [rows,B,A,3], dlogp [rows,B], n_fevals).  d(dlogp)/dt = -div_scale * div
        (reverse_ode: (-b, +div_scale * div) on the descending grid the caller passes), dlogp is written * out_scale."""
        B = self._check_x(x0, "x0")
        on_gpu = hasattr(x0, "data_ptr") and x0.is_cuda
        rd = _rollout_desc(scheme, t_grid, save_every, _lib.MEM_DEVICE if on_gpu else _lib.MEM_HOST, 0.0, 0, 0, False, rtol, atol,
                           step_control=step_control)
        rows = int(_lib.lib().ti_rollout_rows(rd.n_step, rd.save_every))
        out, dl = _alloc_like(x0 if on_gpu else None, (rows, B, self.A, 3)), _alloc_like(x0 if on_gpu else None, (rows, B))
        (xp, cp, op, dp), dev, keep = self._ptrs((x0, (B, self.A, 3), False, "x0"), self._cond_spec(cond, B), (out, None, True, "out"), (dl, None, True, "out_dlogp"))
        nfe = C.c_int64(0)
        _lib.check(_lib.lib().ti_painn_rollout_dlogp(self.h, C.byref(rd), xp, cp, B, float(div_scale), float(out_scale), int(bool(reverse_ode)),
                                                     op, dp, C.byref(nfe)))
        return out, dl, nfe.value

    # ---- Hutchinson's estimate of the divergence (include/ti_hip.h ti_painn_drift_div_est): k Rademacher probes per molecule,
    # keyed by (probe_seed, traj_offset + b, probe); unbiased but noisy -- drift_div / rollout_dlogp stay the exact path
    def drift_div_est(self, x, t, cond=None, n_probes=1, probe_seed=0, traj_offset=0):
        """(b(x) [B,A,3], est [B]) with est = (1/k) sum_p eps_p^T J eps_p, E[est] = div (no 1e-2 factor).  t: a scalar or [B]."""
        B = self._check_x(x)
        like = x if hasattr(x, "data_ptr") and x.is_cuda else None
        out, div = _alloc_like(like, (B, self.A, 3)), _alloc_like(like, (B,))
        tv = self._times(t, B)
        mem = lambda dev: _lib.MEM_DEVICE if dev else _lib.MEM_HOST
        if tv is not None:
            (xp, tp, cp, op, dp), dev, keep = self._ptrs((x, (B, self.A, 3), False, "x"), tv, self._cond_spec(cond, B), (out, None, True, "out"),
                                                         (div, None, True, "out_div"))
            _lib.check(_lib.lib().ti_painn_drift_div_est_tv(self.h, xp, tp, cp, B, int(n_probes), int(probe_seed), int(traj_offset), op, dp, mem(dev)))
            return out, div
        (xp, cp, op, dp), dev, keep = self._ptrs((x, (B, self.A, 3), False, "x"), self._cond_spec(cond, B), (out, None, True, "out"), (div, None, True, "out_div"))
        _lib.check(_lib.lib().ti_painn_drift_div_est(self.h, xp, float(t), cp, B, int(n_probes), int(probe_seed), int(traj_offset), op, dp, mem(dev)))
        return out, div

    def rollout_dlogp_est(self, x0, cond, t_grid, n_probes=1, probe_seed=0, traj_offset=0, scheme="euler", save_every=1, div_scale=1.0,
                          out_scale=1.0, reverse_ode=False, rtol=1e-4, atol=1e-4, step_control="batch"):
        """rollout_dlogp with drift_div_est in place of the exact divergence; the probes of molecule b are those of global id
        traj_offset + b, fixed for the whole call.  Returns (path [rows,B,A,3], dlogp [rows,B], n_fevals)."""
        B = self._check_x(x0, "x0")
        on_gpu = hasattr(x0, "data_ptr") and x0.is_cuda
        rd = _rollout_desc(scheme, t_grid, save_every, _lib.MEM_DEVICE if on_gpu else _lib.MEM_HOST, 0.0, 0, traj_offset, False, rtol, atol,
                           step_control=step_control)
        rows = int(_lib.lib().ti_rollout_rows(rd.n_step, rd.save_every))
        out, dl = _alloc_like(x0 if on_gpu else None, (rows, B, self.A, 3)), _alloc_like(x0 if on_gpu else None, (rows, B))
        (xp, cp, op, dp), dev, keep = self._ptrs((x0, (B, self.A, 3), False, "x0"), self._cond_spec(cond, B), (out, None, True, "out"), (dl, None, True, "out_dlogp"))
        nfe = C.c_int64(0)
        _lib.check(_lib.lib().ti_painn_rollout_dlogp_est(self.h, C.byref(rd), int(n_probes), int(probe_seed), xp, cp, B, float(div_scale),
                                                         float(out_scale), int(bool(reverse_ode)), op, dp, C.byref(nfe)))
        return out, dl, nfe.value

    # ---- parity-test taps
    def debug_tap(self, stage: int):
        _lib.check(_lib.lib().ti_painn_debug_tap(self.h, int(stage)))

    def debug_poison(self, B: int, value: float):
        """Test hook: fill the per-atom accumulators of the workspace for B molecules, the edge state and the parked edge geometry
        with `value` (first-touch accumulators, rows the pair-major kernel skips)."""
        _lib.check(_lib.lib().ti_painn_debug_poison(self.h, int(B), float(value)))

    def debug_phi0_path(self):
        """(path, classes) of the last drift evaluation: path 1 = layer 0 read the phi table, 0 = fallback, -1 = none yet;
        classes = distinct cond classes the call's class pass found (cap + 1: more than the cap; 0: no class pass)."""
        n = np.zeros(1, np.int32)
        path = _lib.lib().ti_painn_debug_phi0_path(self.h, _lib.iptr(n))
        return int(path), int(n[0])

    def debug_pair_blocks(self):
        """(G, nblk, n_tile) of the handle's pair-major template -- molecules per group, row blocks per group, leading tile blocks (the
        rest are general blocks) -- or None when it has none."""
        g, n, t = (np.zeros(1, np.int32) for _ in range(3))
        if _lib.lib().ti_painn_debug_pair_blocks(self.h, _lib.iptr(g), _lib.iptr(n), _lib.iptr(t)) != 1:
            return None
        return int(g[0]), int(n[0]), int(t[0])

    def debug_pair_seeded(self):
        """(path, template) of the seeded accumulators: path 1 = the message launches of the last drift evaluation ran general
        launch first with plain stores, then tiles that only add; 0 = the first-touch order; -1 = none yet.  template 1 = the
        handle's pair template is seeded (its general rows name every atom of a group exactly once), else 0."""
        s = np.zeros(1, np.int32)
        path = _lib.lib().ti_painn_debug_pair_seeded(self.h, _lib.iptr(s))
        return int(path), int(s[0])

    def debug_pair_tails(self):
        """(path, S) of the merged tails: path 1 = the seeded general launches of the last drift evaluation walked super-groups of S
        groups, their last general blocks as one; 0 = one group per wave; -1 = none yet.  S = 0: the template has no such tails."""
        s = np.zeros(1, np.int32)
        path = _lib.lib().ti_painn_debug_pair_tails(self.h, _lib.iptr(s))
        return int(path), int(s[0])

    def debug_embed_path(self):
        """Which embed launch the last drift evaluation ran: 1 = per class (the table path: (class, atom) rows alone, layer 0's
        update reads s through the class map), 0 = every atom, -1 = none yet."""
        return int(_lib.lib().ti_painn_debug_embed_path(self.h))

    def debug_update_keep(self):
        """How many of the three v_eff components the update launches of the last drift evaluation kept in registers: 1..3,
        0 = the builds that park all of it in the dv accumulator (TI_UPDATE_KEEP=0 at creation, f32, fp16 storage, F = 256),
        -1 = none yet."""
        return int(_lib.lib().ti_painn_debug_update_keep(self.h))

    def debug_read(self, what: str, B: int):
        """what: 's' | 'v' | 'e', or 'ts' | 'tv' | 'te' for the tangents of the last jvp() call."""
        shape = {"s": (B, self.A, self.F), "v": (B, self.A, 3, self.F), "e": (B, self.E, self.F)}[what[-1]]
        out = np.empty(shape, np.float32)
        _lib.check(_lib.lib().ti_painn_debug_read(self.h, {"s": 0, "v": 1, "e": 2, "ts": 3, "tv": 4, "te": 5}[what], _lib.fptr(out), out.size))
        return out


class AdwEngine(_Engine):
    """FCNetMultiBeta drift (+ exact divergence) and fixed-step / adaptive integrators: the 1-D double well (dim = 1) and
    FCNetMultiBeta(d, d, H, L) toy systems in d = dim <= 16 dimensions."""

    def __init__(self, hidden, num_layers, flat_weights_f64, device=0, precision="f32", dim=1):
        if precision not in _lib.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_lib.PRECISIONS)}")
        self.hidden, self.num_layers, self.precision, self.dim = int(hidden), int(num_layers), precision, int(dim)
        self.desc = _lib.AdwDesc(self.hidden, self.num_layers, _lib.PRECISIONS[precision])
        w = np.ascontiguousarray(flat_weights_f64, np.float64)
        self.device = int(device)
        if self.dim == 1:
            self.h = _lib.lib().ti_adw_create(C.byref(self.desc), w.ctypes.data_as(C.POINTER(C.c_double)), w.size, self.device)
        else:
            self.h = _lib.lib().ti_adw_create_nd(C.byref(self.desc), self.dim, w.ctypes.data_as(C.POINTER(C.c_double)), w.size, self.device)
        if not self.h:
            raise _lib.TiError(-1, _lib.last_error())

    def _obs_x_shape(self, x):
        B = int(x.shape[0])
        return B, self._xs(B)

    def _xs(self, *lead):
        """shape of a state array: lead dims + (d,) for d > 1; the 1-D engine keeps the flat [.., B] shapes"""
        return tuple(lead) + ((self.dim,) if self.dim > 1 else ())

    def drift(self, x, t, beta0, beta1, out=None, return_div=False):
        """b(x, t) [B] ([B, d] for d > 1); with return_div also the divergence sum_i d b_i / d x_i [B] (reference scaling NOT
        applied).  t: a scalar or one time per row ([B])."""
        B = int(x.shape[0])
        xs = self._xs(B)
        like = x if hasattr(x, "data_ptr") and x.is_cuda else None
        if out is None:
            out = _alloc_like(like, xs)
        div = _alloc_like(like, (B,)) if return_div else None
        tv = self._times(t, B)
        if tv is not None:
            (xp, tp, b0p, b1p, op, dp), dev, keep = self._ptrs((x, xs, False, "x"), tv, (beta0, (B,), False, "beta0"), (beta1, (B,), False, "beta1"),
                                                               (out, xs, True, "out"), (div, None, True, "out_div"))
            _lib.check(_lib.lib().ti_adw_drift_tv(self.h, xp, tp, b0p, b1p, B, op, dp, _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
            return (out, div) if return_div else out
        (xp, b0p, b1p, op, dp), dev, keep = self._ptrs((x, xs, False, "x"), (beta0, (B,), False, "beta0"), (beta1, (B,), False, "beta1"),
                                                       (out, xs, True, "out"), (div, None, True, "out_div"))
        mem = _lib.MEM_DEVICE if dev else _lib.MEM_HOST
        if not return_div:
            _lib.check(_lib.lib().ti_adw_drift(self.h, xp, float(t), b0p, b1p, B, op, mem))
            return out
        _lib.check(_lib.lib().ti_adw_drift_div(self.h, xp, float(t), b0p, b1p, B, op, dp, mem))
        return out, div

    def velocity_loss(self, x0, x1, beta0, beta1, *, kind="standard", gamma="brownian", a=1.0, t=None, t_distr="uniform", z=None, seed=0,
                      traj_offset=0, draw=0, tbins=0, returns=()):
        """ti_adw_vloss: PainnEngine.velocity_loss for particles x0, x1 [B] ([B, d] for d > 1) with per-row beta0, beta1 [B]; no centring;
        mean = sum of loss / B."""
        B = int(x0.shape[0])
        desc = self._vloss_desc(kind, gamma, a, "none", t, t_distr, seed, traj_offset, draw, tbins)
        return self._vloss(False, self._xs(B), x0, x1, [(beta0, (B,), False, "beta0"), (beta1, (B,), False, "beta1")], desc, t, z, returns)

    def interpolate(self, x0, x1, *, kind="standard", gamma="brownian", a=1.0, t=None, t_distr="uniform", z=None, seed=0, traj_offset=0,
                    draw=0):
        """ti_adw_vloss_interp: stage one of velocity_loss alone -> dict: t [B], z (standard), xt [2, ...] (one_sided: [1, ...])."""
        B = int(x0.shape[0])
        desc = self._vloss_desc(kind, gamma, a, "none", t, t_distr, seed, traj_offset, draw, 0)
        return self._vloss(True, self._xs(B), x0, x1, [], desc, t, z, ())

    def rollout(self, x0, beta0, beta1, t_grid, scheme="euler", save_every=1, eps=0.0, seed=0, traj_offset=0, out=None,
                return_dlogp=False, rtol=1e-4, atol=1e-4, step_offset=0, step_control="batch", *, fused=False):
        """(path [rows,B] ([rows,B,d] for d > 1), n_fevals), or (path, dlogp [rows,B] (already * 1e2 like the reference), n_fevals).
        step_control='trajectory' (dopri5 only): every particle gets the steps a batch of one would take (see PainnEngine.rollout).
        fused=True: the whole step loop in one kernel launch (ti_adw_rollout_fused: dim = 1, euler / heun / em, no observer; anything
        else raises TiError with TI_E_UNSUPPORTED) -- the same arrays bit for bit."""
        B = int(x0.shape[0])
        on_gpu = hasattr(x0, "data_ptr") and x0.is_cuda
        rd = _rollout_desc(scheme, t_grid, save_every, _lib.MEM_DEVICE if on_gpu else _lib.MEM_HOST, eps, seed, traj_offset, False, rtol, atol,
                           step_offset, step_control)
        rows = int(_lib.lib().ti_rollout_rows(rd.n_step, rd.save_every))
        if out is None:
            out = _alloc_like(x0 if on_gpu else None, self._xs(rows, B))
        dl = _alloc_like(x0 if on_gpu else None, (rows, B)) if return_dlogp else None
        (xp, b0p, b1p, op, dp), dev, keep = self._ptrs((x0, self._xs(B), False, "x0"), (beta0, (B,), False, "beta0"), (beta1, (B,), False, "beta1"),
                                                       (out, self._xs(rows, B), True, "out"), (dl, None, True, "out_dlogp"))
        nfe = C.c_int64(0)
        if fused:
            _lib.check(_lib.lib().ti_adw_rollout_fused(self.h, C.byref(rd), xp, b0p, b1p, B, op, dp, C.byref(nfe)))
            return (out, dl, nfe.value) if return_dlogp else (out, nfe.value)
        if not return_dlogp:
            _lib.check(_lib.lib().ti_adw_rollout(self.h, C.byref(rd), xp, b0p, b1p, B, op, C.byref(nfe)))
            return out, nfe.value
        _lib.check(_lib.lib().ti_adw_rollout_dlogp(self.h, C.byref(rd), xp, b0p, b1p, B, op, dp, C.byref(nfe)))
        return out, dl, nfe.value


class _Trainer(_Engine):
    """What AdwTrainer and PainnTrainer share: the optimiser entry points ti_{adw,painn}_train_{apply,get_state,set_state,set_lr}
    (`_PREFIX` names the family) and the argument plumbing of their gradient and many-step calls."""
    _PREFIX = None

    def _fn(self, name):
        return getattr(_lib.lib(), f"{self._PREFIX}_{name}")

    def _created(self):
        if not self.h:
            raise _lib.TiError(-1, _lib.last_error())

    def _loss_out(self, B, like):
        """The fp64 [B] loss buffer where `like` lives (None: numpy) and its pointer"""
        if like is not None:
            import torch
            loss = torch.empty(B, dtype=torch.float64, device=like.device)
            return loss, C.c_void_p(loss.data_ptr())
        loss = np.empty(B, np.float64)
        return loss, C.c_void_p(loss.ctypes.data)

    def _index_ptrs(self, idx0, idx1, dev):
        """The pointers of a many-step call's index arrays (None where absent), and what keeps them alive"""
        ip, ikeep = [None, None], []
        for k, idx in enumerate((idx0, idx1)):
            if idx is None:
                continue
            if hasattr(idx, "data_ptr"):
                if not dev or str(idx.dtype) != "torch.int64" or not idx.is_contiguous() or not idx.is_cuda:
                    raise TypeError("index tensors must be contiguous int64 CUDA tensors, with the data on the GPU too")
                ip[k] = C.c_void_p(idx.data_ptr()); ikeep.append(idx)
            else:
                if dev:
                    raise ValueError("all buffers of a call must live in the same memory space (all host or all on the GPU)")
                arr = np.ascontiguousarray(idx, np.int64)
                ip[k] = C.c_void_p(arr.ctypes.data); ikeep.append(arr)
        return ip, ikeep

    def apply(self, g):
        """ti_{adw,painn}_train_apply: clip + Adam with the given fp64 gradient [n_weights] -> True where the step was skipped (non-finite entry)."""
        g = np.ascontiguousarray(g, np.float64).reshape(-1)
        if g.size != self.n_weights:
            raise ValueError(f"g must hold {self.n_weights} entries, got {g.size}")
        skipped = C.c_int32(0)
        _lib.check(self._fn("apply")(self.h, g.ctypes.data_as(C.POINTER(C.c_double)), C.byref(skipped)))
        return bool(skipped.value)

    def state(self):
        """dict(w, m, v [n_weights] float64, n_applied, n_skipped): master weights, Adam moments, counters"""
        w, m, v = (np.empty(self.n_weights, np.float64) for _ in range(3))
        na, ns = C.c_int64(0), C.c_int64(0)
        dp = C.POINTER(C.c_double)
        _lib.check(self._fn("get_state")(self.h, w.ctypes.data_as(dp), m.ctypes.data_as(dp), v.ctypes.data_as(dp), C.byref(na), C.byref(ns)))
        return dict(w=w, m=m, v=v, n_applied=int(na.value), n_skipped=int(ns.value))

    def load_state(self, w=None, m=None, v=None, n_applied=0, **_):
        dp = C.POINTER(C.c_double)
        arrs = []
        for name, a in (("w", w), ("m", m), ("v", v)):
            if a is None:
                arrs.append(None)
                continue
            a = np.ascontiguousarray(a, np.float64).reshape(-1)
            if a.size != self.n_weights:
                raise ValueError(f"{name} must hold {self.n_weights} entries, got {a.size}")
            arrs.append(a)
        ptrs = [None if a is None else a.ctypes.data_as(dp) for a in arrs]
        _lib.check(self._fn("set_state")(self.h, *ptrs, int(n_applied)))

    def set_lr(self, lr):
        _lib.check(self._fn("set_lr")(self.h, float(lr)))
        self.train_desc.lr = float(lr)

    def weights(self):
        """The fp64 master weights in the canonical layout [n_weights]"""
        w = np.empty(self.n_weights, np.float64)
        _lib.check(self._fn("get_state")(self.h, w.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, None))
        return w


class AdwTrainer(_Trainer):
    """FCNetMultiBeta(d, d, H, L) trained on the velocity loss on the device (ti_adw_train_*): fp64 master weights and Adam moments,
    forward / backward / weight gradient on the f32 matrix cores, clip_grad_norm_ + torch.optim.Adam (L2 weight_decay) in fp64, the
    NaN skip of the reference's loop decided on the device.  `flat`: the canonical fp64 weights (weights.flatten_state_dict).
    Arrays are numpy or CUDA tensors as AdwEngine.velocity_loss takes them: x0, x1 [B] ([B, d] for d > 1), beta0, beta1 [B]."""
    _PREFIX = "ti_adw_train"

    def __init__(self, hidden, layers, flat, dim=1, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=1.0, device=0,
                 precision="f32"):
        if precision not in _lib.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_lib.PRECISIONS)}")
        self.hidden, self.num_layers, self.dim, self.device = int(hidden), int(layers), int(dim), int(device)
        self.desc = _lib.AdwDesc(self.hidden, self.num_layers, _lib.PRECISIONS[precision])
        self.train_desc = _lib.AdwTrainDesc(float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), float(max_grad_norm))
        w = np.ascontiguousarray(flat, np.float64).reshape(-1)
        self.n_weights = int(w.size)
        self.h = _lib.lib().ti_adw_trainer_create(C.byref(self.desc), self.dim, w.ctypes.data_as(C.POINTER(C.c_double)), w.size,
                                                  C.byref(self.train_desc), self.device)
        self._created()

    def _xs(self, *lead):
        return tuple(lead) + ((self.dim,) if self.dim > 1 else ())

    def _desc(self, kind, gamma, a, t, t_distr, seed, traj_offset, draw):
        return self._vloss_desc(kind, gamma, a, "none", t, t_distr, seed, traj_offset, draw, 0)

    def grad(self, x0, x1, beta0, beta1, *, kind="standard", gamma="brownian", a=1.0, t=None, t_distr="uniform", z=None, seed=0,
             traj_offset=0, draw=0):
        """ti_adw_train_grad -> dict(loss [B] float64 (where x0 lives), mean, grad [n_weights] float64 numpy, gnorm); no update."""
        B = int(x0.shape[0])
        xs = self._xs(B)
        desc = self._desc(kind, gamma, a, t, t_distr, seed, traj_offset, draw)
        (x0p, x1p, b0p, b1p, tp, zp), dev, keep = self._ptrs((x0, xs, False, "x0"), (x1, xs, False, "x1"), (beta0, (B,), False, "beta0"),
                                                             (beta1, (B,), False, "beta1"), (t, (B,), False, "t"), (z, xs, False, "z"))
        loss, lp = self._loss_out(B, x0 if dev else None)
        g = np.empty(self.n_weights, np.float64)
        mean, gnorm = C.c_double(0.0), C.c_double(0.0)
        _lib.check(_lib.lib().ti_adw_train_grad(self.h, C.byref(desc), x0p, x1p, b0p, b1p, tp, zp, B, lp, C.byref(mean),
                                                g.ctypes.data_as(C.POINTER(C.c_double)), C.byref(gnorm), _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        return dict(loss=loss, mean=mean.value, grad=g, gnorm=gnorm.value)

    def steps(self, x0, x1, beta0, beta1, idx0=None, idx1=None, *, n_steps=None, batch=None, kind="standard", gamma="brownian", a=1.0,
              t=None, t_distr="uniform", z=None, seed=0, traj_offset=0, draw=0):
        """ti_adw_train_steps -> (loss [n_steps] float64 numpy, NaN where skipped; the number of skipped steps).  idx0, idx1
        [n_steps, B] int64 (numpy, or CUDA tensors when the data are): step k trains on rows idx0[k] of (x0, beta0) and idx1[k] of
        (x1, beta1), drawn with draw + k.  Without indices: one step on rows 0 .. batch - 1 (batch defaults to all rows)."""
        n0, n1 = int(x0.shape[0]), int(x1.shape[0])
        specs = [(x0, self._xs(n0), False, "x0"), (x1, self._xs(n1), False, "x1"), (beta0, (n0,), False, "beta0"), (beta1, (n1,), False, "beta1")]
        if (idx0 is None) != (idx1 is None):
            raise ValueError("idx0 and idx1 must both be given or both be None")
        if idx0 is None:
            B, n = int(batch if batch is not None else n0), 1
            if n_steps not in (None, 1):
                raise ValueError("without indices a call makes one step")
        else:
            if tuple(idx0.shape) != tuple(idx1.shape) or len(idx0.shape) != 2:
                raise ValueError("idx0 and idx1 must be [n_steps, B] and equally shaped")
            n, B = int(idx0.shape[0]), int(idx0.shape[1])
        specs += [(t, (B,), False, "t"), (z, self._xs(B), False, "z")]
        (x0p, x1p, b0p, b1p, tp, zp), dev, keep = self._ptrs(*specs)
        ip, ikeep = self._index_ptrs(idx0, idx1, dev)
        desc = self._desc(kind, gamma, a, t, t_distr, seed, traj_offset, draw)
        loss = np.empty(n, np.float64)
        skipped = C.c_int64(0)
        _lib.check(_lib.lib().ti_adw_train_steps(self.h, C.byref(desc), x0p, n0, x1p, n1, b0p, b1p, ip[0], ip[1], tp, zp, B, n,
                                                 loss.ctypes.data_as(C.POINTER(C.c_double)), C.byref(skipped),
                                                 _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        return loss, int(skipped.value)

    def step(self, x0, x1, beta0, beta1, **kw):
        """One optimiser step on the whole batch -> (mean loss, or NaN where the step was skipped; skipped 0 / 1)."""
        loss, skipped = self.steps(x0, x1, beta0, beta1, **kw)
        return float(loss[0]), skipped


class PainnTrainer(_Trainer):
    """cPaiNN trained on the velocity loss on the device (ti_painn_train_*): fp64 master weights and Adam moments, a forward pass
    that keeps its intermediates and the reverse pass through every layer, products on the f32 matrix cores, every reduction over
    rows in fp64, clip_grad_norm_ + torch.optim.Adam (L2 weight_decay) in fp64, the NaN skip decided on the device.  `flat`: the
    canonical fp64 weights (weights.flatten_state_dict with weights.painn_param_spec).  Arrays are numpy or CUDA tensors as
    PainnEngine.velocity_loss takes them: x0, x1 [B, A, 3], cond [B, A, ncond] (None for the single-T variant)."""
    _PREFIX = "ti_painn_train"

    def __init__(self, variant, F, L, A, edge_src, edge_dst, edge_type, atom_ids, flat, *, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                 weight_decay=0.0, max_grad_norm=1.0, max_workspace_bytes=0, n_types=25, temp_length=10.0, time_length=10.0,
                 length_scale=10.0, temperatures=(300, 400, 500, 600, 700, 800, 900, 1000), device=0, precision="f32"):
        if precision not in _lib.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_lib.PRECISIONS)}")
        temps = np.asarray(temperatures, np.float32)
        es, ed, et, ai = (np.ascontiguousarray(a, np.int32) for a in (edge_src, edge_dst, edge_type, atom_ids))
        if not (es.shape == ed.shape == et.shape) or es.ndim != 1 or ai.shape != (A,):
            raise ValueError("edge_src/edge_dst/edge_type must be 1-D and equally long; atom_ids must have A entries")
        self.variant, self.F, self.L, self.A, self.E = int(variant), int(F), int(L), int(A), int(es.size)
        self.ncond = W.N_COND[self.variant]
        self.desc = _lib.PainnDesc(self.variant, self.F, self.L, int(n_types), self.A, self.E, float(temp_length), float(time_length),
                                   float(length_scale), float(temps.mean(dtype=np.float32)), float(temps.max() - temps.min()), _lib.PRECISIONS[precision])
        self.train_desc = _lib.PainnTrainDesc(float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), float(max_grad_norm),
                                              int(max_workspace_bytes))
        w = np.ascontiguousarray(flat, np.float64).reshape(-1)
        self.n_weights, self.device = int(w.size), int(device)
        self.h = _lib.lib().ti_painn_trainer_create(C.byref(self.desc), w.ctypes.data_as(C.POINTER(C.c_double)), w.size, _lib.iptr(es), _lib.iptr(ed),
                                                    _lib.iptr(et), _lib.iptr(ai), C.byref(self.train_desc), self.device)
        self._created()

    def _call_args(self, x0, x1, cond, t, z):
        B = int(x0.shape[0])
        xs = (B, self.A, 3)
        if (cond is None) != (self.ncond == 0):
            raise ValueError(f"this variant takes {'no cond' if self.ncond == 0 else f'cond [B, A, {self.ncond}]'}")
        ptrs, dev, keep = self._ptrs((x0, xs, False, "x0"), (x1, xs, False, "x1"), (cond, (B, self.A, self.ncond), False, "cond"),
                                     (t, (B,), False, "t"), (z, xs, False, "z"))
        return B, ptrs, dev, keep

    def grad(self, x0, x1, cond=None, *, kind="standard", gamma="brownian", a=1.0, center="batch", t=None, t_distr="uniform", z=None, seed=0,
             traj_offset=0, draw=0):
        """ti_painn_train_grad -> dict(loss [B] float64 (where x0 lives), mean, grad [n_weights] float64 numpy, gnorm); no update."""
        desc = self._vloss_desc(kind, gamma, a, center, t, t_distr, seed, traj_offset, draw, 0)
        B, (x0p, x1p, cp, tp, zp), dev, keep = self._call_args(x0, x1, cond, t, z)
        loss, lp = self._loss_out(B, x0 if dev else None)
        g = np.empty(self.n_weights, np.float64)
        mean, gnorm = C.c_double(0.0), C.c_double(0.0)
        _lib.check(_lib.lib().ti_painn_train_grad(self.h, C.byref(desc), x0p, x1p, cp, tp, zp, B, lp, C.byref(mean),
                                                  g.ctypes.data_as(C.POINTER(C.c_double)), C.byref(gnorm), _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        return dict(loss=loss, mean=mean.value, grad=g, gnorm=gnorm.value)

    def step(self, x0, x1, cond=None, *, kind="standard", gamma="brownian", a=1.0, center="batch", t=None, t_distr="uniform", z=None, seed=0,
             traj_offset=0, draw=0):
        """ti_painn_train_step: one optimiser step on the batch -> (mean loss, or NaN where the step was skipped; skipped 0 / 1)."""
        desc = self._vloss_desc(kind, gamma, a, center, t, t_distr, seed, traj_offset, draw, 0)
        B, (x0p, x1p, cp, tp, zp), dev, keep = self._call_args(x0, x1, cond, t, z)
        mean, skipped = C.c_double(0.0), C.c_int32(0)
        _lib.check(_lib.lib().ti_painn_train_step(self.h, C.byref(desc), x0p, x1p, cp, tp, zp, B, C.byref(mean), C.byref(skipped),
                                                  _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        return mean.value, int(skipped.value)

    def steps(self, x0, x1, temp0=None, temp1=None, idx0=None, idx1=None, *, batch=None, update=True, noise="given", track_best=False,
              kind="standard", gamma="brownian", a=1.0, center="batch", t_distr="uniform", seed=0, traj_offset=0, draw=0):
        """ti_painn_train_steps -> (loss [n_steps] float64 numpy, NaN where skipped; the number of skipped steps).  x0 [n0, A, 3] and
        x1 [n1, A, 3] are the resident sets, temp0 [n0] and temp1 [n1] their temperatures (ambient: both, multi-T latent: temp1,
        single-T: neither); idx0, idx1 [n_steps, B] int64 (numpy, or CUDA tensors when the data are): step k takes rows idx0[k] of set 0
        and idx1[k] of set 1 and is drawn with draw + k.  Without indices: one step on rows 0 .. batch - 1.  update=False: forward
        only, the mean loss of every minibatch at the current weights.  noise="drawn" | "aligned" (one-sided loss, x0 None): the
        minibatch's x0 is drawn on the device as `noise` does.  track_best: keep the weights of the step with the smallest loss
        (`best`).  One host synchronisation, at the end."""
        if noise not in _lib.PAINN_NOISES:
            raise ValueError(f"noise must be one of {sorted(_lib.PAINN_NOISES)}, got {noise!r}")
        given = noise == "given"
        if given == (x0 is None):
            raise ValueError("noise='given' takes x0; a drawn noise takes x0=None")
        n1 = int(x1.shape[0])
        n0 = int(x0.shape[0]) if given else n1
        if (idx0 is None) != (idx1 is None) and given:
            raise ValueError("idx0 and idx1 must both be given or both be None")
        if idx0 is None and not given:
            idx0 = idx1                                  # the values of idx0 are not read without a set 0
        if idx1 is None:
            n, B = 1, int(batch if batch is not None else min(n0, n1))
        else:
            if tuple(idx0.shape) != tuple(idx1.shape) or len(idx1.shape) != 2:
                raise ValueError("idx0 and idx1 must be [n_steps, B] and equally shaped")
            n, B = int(idx1.shape[0]), int(idx1.shape[1])
        (x0p, x1p, t0p, t1p), dev, keep = self._ptrs((x0, (n0, self.A, 3), False, "x0"), (x1, (n1, self.A, 3), False, "x1"),
                                                     (temp0, (n0,), False, "temp0"), (temp1, (n1,), False, "temp1"))
        ip, ikeep = self._index_ptrs(idx0, idx1, dev)
        desc = self._vloss_desc(kind, gamma, a, center, None, t_distr, seed, traj_offset, draw, 0)
        sd = _lib.PainnStepsDesc(n, int(bool(update)), _lib.PAINN_NOISES[noise], int(bool(track_best)))
        loss = np.empty(n, np.float64)
        skipped = C.c_int64(0)
        _lib.check(_lib.lib().ti_painn_train_steps(self.h, C.byref(desc), C.byref(sd), x0p, n0, t0p, x1p, n1, t1p, ip[0], ip[1], B,
                                                   loss.ctypes.data_as(C.POINTER(C.c_double)), C.byref(skipped),
                                                   _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        return loss, int(skipped.value)

    def noise(self, x1=None, *, B=None, aligned=False, seed=0, traj_offset=0, draw=0, return_rot=False):
        """ti_painn_train_noise: the latent base samples of B molecules -> x0 [B, A, 3] float32 (where x1 lives; numpy without x1), and
        with return_rot the rotations [B, 3, 3] float64.  Drawn as N(seed, traj_offset + b, draw, 3 a + c), centred per molecule;
        aligned=True rotates each onto its x1 by the proper rotation that minimises sum_a |x1_a - R x0_a|^2."""
        if x1 is None and (aligned or B is None):
            raise ValueError("aligned noise needs x1; without x1 pass B")
        B = int(x1.shape[0]) if x1 is not None else int(B)
        (x1p,), dev, keep = self._ptrs((x1, (B, self.A, 3), False, "x1"))
        rot = None
        if dev:
            import torch
            out = torch.empty((B, self.A, 3), dtype=torch.float32, device=x1.device)
            op = C.c_void_p(out.data_ptr())
            if return_rot and aligned:
                rot = torch.empty((B, 3, 3), dtype=torch.float64, device=x1.device)
            rp = C.c_void_p(rot.data_ptr()) if rot is not None else None
        else:
            out = np.empty((B, self.A, 3), np.float32)
            op = C.c_void_p(out.ctypes.data)
            if return_rot and aligned:
                rot = np.empty((B, 3, 3), np.float64)
            rp = C.c_void_p(rot.ctypes.data) if rot is not None else None
        _lib.check(_lib.lib().ti_painn_train_noise(self.h, int(seed), int(traj_offset), int(draw), x1p if aligned else None, B,
                                                   _lib.PAINN_NOISES["aligned" if aligned else "drawn"], op, rp,
                                                   _lib.MEM_DEVICE if dev else _lib.MEM_HOST))
        return (out, rot) if return_rot else out

    def best(self, reset=False):
        """ti_painn_train_best -> dict(w [n_weights] float64 | None, loss, step): the master weights BEFORE the update of the step
        with the smallest loss tracked since the last reset (steps(track_best=True)), that loss, and the step's 0-based count since
        the reset (w None, step -1 where every tracked step was skipped).  reset=True then forgets them."""
        w = np.empty(self.n_weights, np.float64)
        loss, step = C.c_double(0.0), C.c_int64(0)
        _lib.check(_lib.lib().ti_painn_train_best(self.h, w.ctypes.data_as(C.POINTER(C.c_double)), C.byref(loss), C.byref(step), int(bool(reset))))
        return dict(w=w if step.value >= 0 else None, loss=loss.value, step=int(step.value))

    def set_graphs(self, n_atoms=None, mask=None, pair_type=None):
        """ti_painn_train_set_graphs: a table of n per-molecule graphs over this trainer's template, as PainnEngine.set_molecules takes
        them: n_atoms [n] in 1..A (None: all A; atoms a >= n_atoms[b] are pad atoms, whose x0 / x1 / cond / z entries are never read),
        mask [n, A] uint32 or int32, bit s of mask[b, d] set when the edge s -> d exists (None: every template edge between real
        atoms), pair_type [n, A, A] in 0..3 at [b, s, d] (None: the template's types).  grad / step then take B = n molecules, molecule
        b on row b; steps (noise='given') takes n = n0 and reads row idx0[k, j].  All None clears the table.  Numpy arrays (or CPU
        tensors) are copied from the host; CUDA tensors, all of them then, are read on the device."""
        L = _lib.lib()
        given = [a for a in (n_atoms, mask, pair_type) if a is not None]
        if not given:
            _lib.check(L.ti_painn_train_set_graphs(self.h, None, None, None, 0, _lib.MEM_HOST))
            return
        on_gpu = [hasattr(a, "data_ptr") and a.is_cuda for a in given]
        if any(on_gpu) != all(on_gpu):
            raise ValueError("all arrays of a call must live in the same memory space (all host or all on the GPU)")
        n = int(given[0].shape[0]) if hasattr(given[0], "shape") else len(given[0])
        shapes = ((n,), (n, self.A), (n, self.A, self.A))
        names = ("n_atoms", "mask", "pair_type")
        if all(on_gpu):
            import torch
            want = (("torch.int32",), ("torch.int32", "torch.uint32"), ("torch.uint8",))
            ptrs, keep = [], []
            for a, shape, name, dts in zip((n_atoms, mask, pair_type), shapes, names, want):
                if a is None:
                    ptrs.append(None)
                    continue
                if str(a.dtype) not in dts:
                    raise TypeError(f"{name} must be {' or '.join(dts)}, got {a.dtype}")
                if tuple(a.shape) != shape:
                    raise ValueError(f"{name} must be {list(shape)}, got {tuple(a.shape)}")
                if a.device.index != self.device:
                    raise ValueError(f"{name} lives on cuda:{a.device.index} but this trainer was created on device {self.device}")
                a = a.contiguous()
                keep.append(a); ptrs.append(C.c_void_p(a.data_ptr()))
            torch.cuda.current_stream(self.device).synchronize()
            _lib.check(L.ti_painn_train_set_graphs(self.h, *ptrs, n, _lib.MEM_DEVICE))
            return
        host = lambda a: a.detach().numpy() if hasattr(a, "data_ptr") else np.asarray(a)
        na = m = t = None
        if n_atoms is not None:
            na = np.ascontiguousarray(host(n_atoms), np.int32)
            if na.shape != shapes[0]:
                raise ValueError(f"n_atoms must be [{n}], got {na.shape}")
        if mask is not None:
            m = host(mask)
            if m.dtype not in (np.uint32, np.int32):
                raise TypeError(f"mask must be uint32 or int32, got {m.dtype}")
            if m.shape != shapes[1]:
                raise ValueError(f"mask must be [{n},{self.A}], got {m.shape}")
            m = np.ascontiguousarray(m.view(np.uint32))
        if pair_type is not None:
            t = host(pair_type)
            if t.shape != shapes[2]:
                raise ValueError(f"pair_type must be [{n},{self.A},{self.A}], got {t.shape}")
            if t.size and (t.min() < 0 or t.max() > 255):
                raise ValueError("pair_type entries must be in 0..3")
            t = np.ascontiguousarray(t, np.uint8)
        ptr = lambda a: None if a is None else C.c_void_p(a.ctypes.data)
        _lib.check(L.ti_painn_train_set_graphs(self.h, ptr(na), ptr(m), ptr(t), n, _lib.MEM_HOST))

    def workspace_bytes(self, B, kind="standard"):
        """ti_painn_train_workspace_bytes: what a call over B molecules needs beside the trainer's state"""
        n = int(_lib.lib().ti_painn_train_workspace_bytes(self.h, int(B), _lib.VLOSS_KINDS[kind]))
        if n < 0:
            raise _lib.TiError(n, _lib.last_error())
        return n


def selftest(device: int = 0):
    _lib.check(_lib.lib().ti_selftest(int(device)))
