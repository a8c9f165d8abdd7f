"""ti_obs_eigh on the GPU: the 45 matrices of tests/eigh_numpy.py (n in {1, 2, 3, 15, 16, 17, 33, 63, 64} x random, Gram-like,
3 I, four-fold degenerate, rank one) against numpy.linalg.eigh(UPLO="U") under the bounds of tests/test_eigh_host.py -- eigenvalues
and max |A V - V diag(w)| within 32 n 2^-53 ||A||_F, max |V^H V - I| within 32 n 2^-53 --, the sweep counts, the triangle that is
read, determinism (position in the batch, n_mat, mem, repetition) and the refusal found on the device.  Worst observed on one
MI355X over the 45 matrices: 4.3, 1.5 and 5.7 of those units; sweep counts within one of the restatement's."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg
import eigh_numpy as en

pytestmark = pytest.mark.gpu
FACTOR = 32.0


@pytest.fixture(scope="module")
def eng():
    return pkg().observables._service_engine(0)


def bits(*arrays):
    return [np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "data_ptr") else a).view(np.uint8).tobytes() for a in arrays]


@pytest.mark.parametrize("n", en.SIZES)
def test_the_45_matrices_against_lapack(eng, n):
    obs = pkg().observables
    A = np.stack([en.make(kind, n) for kind in en.KINDS])
    w, v, sweeps = obs.eigh_batched(A, engine=eng)
    assert w.shape == (5, n) and v.shape == (5, n, n) and v.dtype == np.complex128 and sweeps.shape == (5,) and sweeps.dtype == np.int32
    worst = np.zeros(3)
    for i, kind in enumerate(en.KINDS):
        err = np.array(en.errors(A[i], w[i], v[i]))
        _, _, ref_sweeps = en.eigh(A[i])
        print(f"{kind}-n{n}: sweeps {sweeps[i]} (restatement {ref_sweeps}), eigenvalues {err[0]:.2f}, residual {err[1]:.2f} (n eps ||A||_F), "
              f"orthogonality {err[2]:.2f} (n eps)")
        worst = np.maximum(worst, err)
        assert (np.diff(w[i]) >= 0).all() and 1 <= sweeps[i] <= 64
        assert (err <= FACTOR).all(), (kind, n, err)
        if kind == "identity":
            assert sweeps[i] == 1 and np.array_equal(w[i], np.full(n, 3.0)) and np.array_equal(v[i], np.eye(n))
    print(f"n = {n}: worst ratios (eigenvalues, residual, orthogonality) {worst}")
    w2, v2, _ = obs.eigh_batched(A, vectors=False, engine=eng)
    assert v2 is None and bits(w2) == bits(w)


def test_diagonal_matrices_take_one_sweep_and_ties_keep_their_position(eng):
    obs = pkg().observables
    d = np.array([2.0, -1.0, 2.0, 0.0, -1.0, 7.5, 2.0])
    w, v, sweeps = obs.eigh_batched(np.diag(d).astype(np.complex128), engine=eng)
    order = np.argsort(d, kind="stable")
    assert int(sweeps) == 1 and np.array_equal(w, d[order]) and np.array_equal(v, np.eye(7)[:, order])


def test_only_the_upper_triangle_is_read(eng):
    obs = pkg().observables
    for n in (17, 64):
        A = en.make("random", n)
        dirty = A.copy()
        dirty[np.tril_indices(n, -1)] = np.nan
        dirty.imag[np.diag_indices(n)] = np.nan                      # the imaginary part of the diagonal is not read either
        assert bits(*obs.eigh_batched(A, engine=eng)) == bits(*obs.eigh_batched(dirty, engine=eng))


def test_a_matrix_gives_the_same_bits_wherever_it_stands(eng):
    """601 matrices of n = 64: more than two per CU, so a second wave of workgroups runs."""
    import torch
    obs = pkg().observables
    rs = np.random.RandomState(5)
    x = rs.standard_normal((601, 64, 64)) + 1j * rs.standard_normal((601, 64, 64))
    A = x + x.conj().transpose(0, 2, 1)
    probe = en.make("gram", 64)
    pos = [0, 255, 256, 600]
    A[pos] = probe
    w, v, sweeps = obs.eigh_batched(A, engine=eng)
    assert (sweeps >= 1).all() and (sweeps <= 64).all()
    one = bits(*obs.eigh_batched(probe[None], engine=eng))
    for i in pos:
        assert bits(w[i:i + 1], v[i:i + 1], sweeps[i:i + 1]) == one, i
    assert bits(*obs.eigh_batched(A, engine=eng)) == bits(w, v, sweeps)                      # a call repeats
    dw, dv, ds = obs.eigh_batched(torch.from_numpy(A).cuda(), engine=eng)                    # device memory
    assert dw.is_cuda and dv.is_cuda and ds.is_cuda and dv.dtype == torch.complex128
    assert bits(dw, dv, ds) == bits(w, v, sweeps)
    err = np.array(en.errors(A[300], w[300], v[300]))
    assert (err <= FACTOR).all(), err


def test_a_non_finite_matrix_is_named_and_nothing_is_written(eng):
    ti = pkg()
    A = np.stack([en.make("random", 16) for _ in range(5)])
    A[3, 2, 9] = np.nan
    with pytest.raises(ti._lib.TiError, match="non-finite entry in matrix 3") as ei:
        ti.observables.eigh_batched(A, engine=eng)
    assert ei.value.code == ti._lib.TI_E_NAN
    a = np.ascontiguousarray(A).view(np.float64).reshape(5, 16, 16, 2)
    w, v, sw = np.full((5, 16), 7.0), np.full((5, 16, 16, 2), 7.0), np.full(5, 7, np.int32)
    vp = lambda x: C.c_void_p(x.ctypes.data)
    rc = ti._lib.lib().ti_obs_eigh(eng.h, vp(a), 5, 16, vp(w), vp(v), vp(sw), ti._lib.MEM_HOST)
    assert rc == ti._lib.TI_E_NAN and "matrix 3" in ti._lib.last_error()
    assert (w == 7.0).all() and (v == 7.0).all() and (sw == 7).all()
    A[3, 9, 2] = np.inf                                              # below the diagonal: not read
    A[3, 2, 9] = 0.5
    w, _, _ = ti.observables.eigh_batched(A, engine=eng)
    assert np.isfinite(w).all()
