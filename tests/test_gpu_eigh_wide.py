"""ti_obs_eigh_wide and ti_obs_gedmd_spectrum_wide on the GPU.  The blocked solver against numpy.linalg.eigh(UPLO="U") under the bounds
of tests/test_eigh_host.py -- eigenvalues and max |A V - V diag(w)| within 32 n 2^-53 ||A||_F, max |V^H V - I| within 32 n 2^-53 -- for
n in {65, 66, 96, 97, 129} x the five kinds of tests/eigh_numpy.py, n = 300 x {random, Gram-like, degenerate} and one random matrix of
n = 1024 (the 20-decade Gram-like kind's orthogonality grows with the sweep count and is unmeasured at that order); the outer sweep
counts beside the restatement's (tests/eigh_wide_numpy.py); n <= 64 through the wide entry against ti_obs_eigh bit for bit; the
triangle that is read; determinism across a launch boundary, repetition and memory modes; the refusal found on the device; and the
generator spectra through tests/golden/gedmd_wide_reference.npz and against the host route on the same Gram stack.  Worst observed
on one MI355X, in the units of eigh_numpy.errors (bound 32): 8.0 / 1.9 / 12.2 over the 25 matrices, 6.3 / 0.9 / 19.4 at n = 300
(Gram-like, 31 outer sweeps), 0.3 / 0.03 / 5.1 at n = 1024 (13 outer sweeps); outer sweep counts within two of the restatement's;
spectra within 1.9e-10 of the reference and 9.6e-11 of the host route (allowed 6.6e-9)."""
import ctypes as C

import numpy as np
import pytest

from conftest import pkg
import eigh_numpy as en
import eigh_wide_numpy as ew
from test_gedmd_wide_host import fixture_cases

pytestmark = pytest.mark.gpu
FACTOR = 32.0


@pytest.fixture(scope="module")
def eng():
    return pkg().observables._service_engine(0)


def bits(*arrays):
    return [np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "data_ptr") else a).view(np.uint8).tobytes() for a in arrays]


def check(A, w, v, sweeps, label):
    err = np.array(en.errors(A, w, v))
    print(f"{label}: outer sweeps {sweeps}, eigenvalues {err[0]:.2f}, residual {err[1]:.2f} (n eps ||A||_F), orthogonality {err[2]:.2f} (n eps)")
    assert (np.diff(w) >= 0).all() and 1 <= sweeps <= 64
    assert (err <= FACTOR).all(), (label, err)
    return err


@pytest.mark.parametrize("n", ew.SIZES)
def test_the_25_matrices_against_lapack(eng, n):
    obs = pkg().observables
    A = np.stack([en.make(kind, n) for kind in en.KINDS])
    w, v, sweeps = obs.eigh_batched_wide(A, engine=eng)
    assert w.shape == (5, n) and v.shape == (5, n, n) and v.dtype == np.complex128 and sweeps.shape == (5,) and sweeps.dtype == np.int32
    worst = np.zeros(3)
    for i, kind in enumerate(en.KINDS):
        worst = np.maximum(worst, check(A[i], w[i], v[i], sweeps[i], f"{kind}-n{n} (restatement {ew.SWEEPS[n][i]} sweeps)"))
        if kind == "identity":
            assert sweeps[i] == 1 and np.array_equal(w[i], np.full(n, 3.0)) and np.array_equal(v[i], np.eye(n))
    print(f"n = {n}: worst ratios (eigenvalues, residual, orthogonality) {worst}")
    w2, v2, _ = obs.eigh_batched_wide(A, vectors=False, engine=eng)
    assert v2 is None and bits(w2) == bits(w)


def test_n_300(eng):
    A = np.stack([en.make(kind, 300) for kind in ("random", "gram", "degenerate")])
    w, v, sweeps = pkg().observables.eigh_batched_wide(A, engine=eng)
    for i, kind in enumerate(("random", "gram", "degenerate")):
        check(A[i], w[i], v[i], sweeps[i], f"{kind}-n300")


def test_n_1024(eng):
    A = en.make("random", 1024)
    w, v, sweeps = pkg().observables.eigh_batched_wide(A, engine=eng)
    check(A, w, v, int(sweeps), "random-n1024")


@pytest.mark.parametrize("n", [17, 64])
def test_narrow_orders_through_the_wide_entry_are_the_narrow_call(eng, n):
    obs = pkg().observables
    A = np.stack([en.make(kind, n) for kind in en.KINDS])
    assert bits(*obs.eigh_batched_wide(A, engine=eng)) == bits(*obs.eigh_batched(A, engine=eng))


def test_only_the_upper_triangle_is_read(eng):
    obs = pkg().observables
    n = 97
    A = en.make("random", n)
    dirty = A.copy()
    dirty[np.tril_indices(n, -1)] = np.nan
    dirty.imag[np.diag_indices(n)] = np.nan                          # the imaginary part of the diagonal is not read either
    assert bits(*obs.eigh_batched_wide(A, engine=eng)) == bits(*obs.eigh_batched_wide(dirty, engine=eng))


def test_a_matrix_gives_the_same_bits_wherever_it_stands(eng):
    """n = 65, one matrix more than a launch holds; identity and Gram-like matrices among random ones, so matrices finish at different
    outer sweeps and their workgroups drop out while the probe's go on."""
    import torch
    ti = pkg()
    obs, n = ti.observables, 65
    cap = ti._lib.eigh_wide_launch_max(n)
    assert cap == 512 and ti._lib.eigh_wide_launch_max(1024) == 64 and ti._lib.eigh_wide_launch_max(1025) == 0
    N = cap + 1
    rs = np.random.RandomState(5)
    x = rs.standard_normal((N, n, n)) + 1j * rs.standard_normal((N, n, n))
    A = x + x.conj().transpose(0, 2, 1)
    A[1::7] = en.make("identity", n)
    A[2::7] = en.make("gram", n, seed=1)
    probe = en.make("gram", n)
    pos = [0, cap - 1, cap, N - 1]
    A[pos] = probe
    w, v, sweeps = obs.eigh_batched_wide(A, engine=eng)
    assert (sweeps >= 1).all() and (sweeps <= 64).all() and len(set(sweeps.tolist())) >= 3
    one = bits(*obs.eigh_batched_wide(probe[None], engine=eng))
    for i in pos:
        assert bits(w[i:i + 1], v[i:i + 1], sweeps[i:i + 1]) == one, i
    assert bits(*obs.eigh_batched_wide(A, engine=eng)) == bits(w, v, sweeps)                 # a call repeats
    dw, dv, ds = obs.eigh_batched_wide(torch.from_numpy(A).cuda(), engine=eng)               # device memory
    assert dw.is_cuda and dv.is_cuda and ds.is_cuda and dv.dtype == torch.complex128
    assert bits(dw, dv, ds) == bits(w, v, sweeps)
    check(A[300], w[300], v[300], sweeps[300], "a random matrix of the stack")


def test_a_non_finite_matrix_is_named_and_nothing_is_written(eng):
    ti = pkg()
    n = 66
    A = np.stack([en.make("random", n) for _ in range(5)])
    A[3, 2, 40] = np.nan
    with pytest.raises(ti._lib.TiError, match="non-finite entry in matrix 3") as ei:
        ti.observables.eigh_batched_wide(A, engine=eng)
    assert ei.value.code == ti._lib.TI_E_NAN
    a = np.ascontiguousarray(A).view(np.float64).reshape(5, n, n, 2)
    w, v, sw = np.full((5, n), 7.0), np.full((5, n, n, 2), 7.0), np.full(5, 7, np.int32)
    vp = lambda x: C.c_void_p(x.ctypes.data)
    rc = ti._lib.lib().ti_obs_eigh_wide(eng.h, vp(a), 5, n, vp(w), vp(v), vp(sw), ti._lib.MEM_HOST)
    assert rc == ti._lib.TI_E_NAN and "matrix 3" in ti._lib.last_error()
    assert (w == 7.0).all() and (v == 7.0).all() and (sw == 7).all()
    A[3, 40, 2] = np.inf                                             # below the diagonal: not read
    A[3, 2, 40] = 0.5
    w, _, _ = ti.observables.eigh_batched_wide(A, engine=eng)
    assert np.isfinite(w).all()


def test_narrow_spectra_through_the_wide_entry_are_the_narrow_call(eng):
    obs = pkg().observables
    rs = np.random.RandomState(3)
    x = rs.standard_normal(4000).astype(np.float32)
    omega = obs.sample_rff_gaussian(1, 50, 0.6, 2)
    G = obs.rff_gram(x, omega, n_boot=3, seed=1, engine=eng)
    assert bits(*obs.gedmd_spectrum_wide(G, omega, 2.0, 4, 1e-4, engine=eng)) == bits(*obs.gedmd_spectrum(G, omega, 2.0, 4, 1e-4, solver="device", engine=eng))


def test_wide_spectra_give_the_same_bits_from_host_and_device_memory(eng):
    """p = 66 (the first blocked order), d = 2, nev = 3 on the two Gram matrices of rff_gram_wide over 200 samples with one resample:
    eigenvalues, eigenvectors and ranks of a call on host arrays against the call on the device stack, so that the per-matrix
    offsets of all three outputs count; without the eigenvectors the eigenvalues and ranks keep their bits."""
    import torch
    obs = pkg().observables
    x = np.random.RandomState(66).standard_normal((200, 2)).astype(np.float32)
    omega = obs.sample_rff_gaussian(2, 66, 0.8, 4)
    Gd = obs.rff_gram_wide(torch.from_numpy(x).cuda(), omega, n_boot=1, seed=3, engine=eng)
    assert Gd.is_cuda and tuple(Gd.shape) == (2, 66, 66)
    G = Gd.cpu().numpy()
    ev, vec, rank = eng.gedmd_spectrum_wide(G, omega, 1.6, 3, 1e-4)
    evd, vecd, rankd = eng.gedmd_spectrum_wide(Gd, omega, 1.6, 3, 1e-4)
    assert evd.is_cuda and vecd.is_cuda and rankd.is_cuda and vecd.dtype == torch.complex128
    assert ev.shape == (2, 3) and vec.shape == (2, 66, 3) and rank.shape == (2,) and rank.dtype == np.int32
    assert np.isfinite(ev).all() and np.isfinite(vec).all() and (rank >= 3).all() and (rank <= 66).all()
    assert bits(evd, vecd, rankd) == bits(ev, vec, rank)
    assert bits(ev[0]) != bits(ev[1])                                # two different matrices
    ev2, none, rank2 = eng.gedmd_spectrum_wide(G, omega, 1.6, 3, 1e-4, vectors=False)
    assert none is None and bits(ev2, rank2) == bits(ev, rank)


def test_fixture_rows_reproduce_the_reference_and_the_host_route(eng):
    """gedmd_generator_wide with the reference's own index rows (p = 300 twice, 513, 130 and the narrower cases): eigenvalues within
    64 ev_dev of the recorded ones, ranks exactly; and gedmd_spectrum_wide on the device Gram stack against gedmd_spectrum(solver="host")
    on the same stack under the same allowance."""
    import torch
    obs = pkg().observables
    cases, ev_dev, _ = fixture_cases()
    worst = [0.0, 0.0]
    for c in cases:
        res = obs.gedmd_generator_wide(c["x"], c["omega"], c["nev"], c["a"], tol=c["tol"], n_boot=3, indices=c["idx"], engine=eng)
        got = np.concatenate([res.eigenvalues[None], res.estimates])
        G = obs.rff_gram_wide(torch.from_numpy(c["x"]).cuda(), c["omega"], n_boot=3, indices=torch.from_numpy(c["idx"]).cuda(), engine=eng)
        d, W, r = obs.gedmd_spectrum_wide(G, c["omega"], c["a"], c["nev"], c["tol"], engine=eng)
        dh, _, rh = obs.gedmd_spectrum(G, c["omega"], c["a"], c["nev"], c["tol"], solver="host")
        dev = (np.abs(got - c["ev"]).max(), np.abs(d - dh).max())
        print(f"{c['name']}: against the reference {dev[0]:.2e}, against the host route {dev[1]:.2e} (64 ev_dev = {64 * ev_dev:.2e}), ranks {r.tolist()}")
        worst = [max(worst[0], dev[0]), max(worst[1], dev[1])]
        assert res.rank == c["rank"][0] and res.eigenvectors.shape == (c["p"], c["nev"])
        np.testing.assert_array_equal(r, c["rank"])
        np.testing.assert_array_equal(r, rh)
        assert W.shape == (4, c["p"], c["nev"]) and np.isfinite(W).all()
        assert dev[0] <= 64 * ev_dev and dev[1] <= 64 * ev_dev, (c["name"], dev)
    print(f"wide device route: worst against the reference {worst[0]:.2e}, against the host route {worst[1]:.2e}")
