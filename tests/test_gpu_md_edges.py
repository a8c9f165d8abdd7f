"""ti_obs_ff_langevin beyond 64 components and with 64-bit keys, against the numpy restatement (tests/ff_forces_numpy.py) through the
checks of tests/test_gpu_md.py.  A lane of the kernel owns the components lane and lane + 64; the second exists only for A >= 22, and
the runs of tests/test_gpu_md.py stop at A = 9.  Here: trajectory parity at A = 25 (the tree fixture: three torsion chunks inside the
step loop) and A = 22 (the dense hub case), the bitwise contract at A = 25, every table at its cap inside the integrator, replica ids and
a seed beyond 32 bits, and the step index's low 32 bits.  All at dt = 0.01 fs, where the restatement stays bounded under the fixtures'
Lennard-Jones contacts (tests/test_ff_forces_host.py test_md_edge_runs_stay_bounded_and_conditioned asserts it: that makes the
comparison meaningful).

Measured ratios, MI355X: profiles/md_parity.txt."""
import numpy as np
import pytest

from conftest import pkg
import ff_forces_numpy as ffn
from test_gpu_forcefield import engine
from test_ff_forces_host import md_edge_case, BIG_IDS, BIG_SEED
from test_gpu_md import LD, bits, check_trajectory, check_bits, run, same

pytestmark = pytest.mark.gpu


def loaded(name):
    ff, m, pos, T, ids, to_nm, kw = md_edge_case(name)
    eng = engine(pos.shape[1])
    eng.set_forcefield(pkg().forcefield.ForceField(**ff, masses=m))
    return eng, ff, m, pos, T, ids, to_nm, kw


def needs_long_double():
    if np.finfo(LD).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than float64 here: d64 cannot be formed")


@pytest.mark.parametrize("name", ["A25", "hub"])
def test_trajectory_parity_beyond_64_components(name):
    """B = 5, 16 steps, stride 4, friction 1 / ps, drawn velocities (components 3A + c up to 149 at A = 25)"""
    needs_long_double()
    eng, ff, m, pos, T, ids, to_nm, kw = loaded(name)
    assert 3 * pos.shape[1] > 64 and kw["dt"] == 1e-5 and kw["n_steps"] == 16 and kw["stride"] == 4 and len(pos) == 5
    check_trajectory(name, eng, ff, m, pos, T, ids, to_nm, kw)


def test_bitwise_contract_at_25_atoms():
    pytest.importorskip("torch")
    eng, ff, m, pos, T, ids, to_nm, kw = loaded("A25")
    check_bits(eng, pos, T, ids, to_nm, strides=(3, 5), dt=kw["dt"])


def test_every_table_at_its_cap_inside_the_integrator():
    """4 steps of the all-caps case: the kernel's LDS at its largest, eight torsion chunks a step"""
    needs_long_double()
    eng, ff, m, pos, T, ids, to_nm, kw = loaded("all_caps")
    assert [len(ff[k]) for k in ("bond_idx", "angle_idx", "torsion_idx")] == [64, 128, 512] and kw["n_steps"] == 4
    check_trajectory("all_caps", eng, ff, m, pos, T, ids, to_nm, kw)


def test_64_bit_replica_ids_and_seed():
    needs_long_double()
    eng, ff, m, pos, T, ids, to_nm, kw = loaded("A9_ids")
    assert ids.tolist() == [7, 2 ** 32 + 1, 2 ** 40 + 9, 2 ** 62 + 3, -2] and kw["seed"] == 2 ** 40 + 11
    check_trajectory("A9_ids", eng, ff, m, pos, T, ids, to_nm, kw)
    # the keys' upper halves enter: the low 32 bits alone give other velocities
    v_big = ffn.draw_velocities(T, ids, m, kw["seed"], 0)
    assert (v_big[1:] != ffn.draw_velocities(T, ids % 2 ** 32, m, kw["seed"], 0)[1:]).all()
    assert (v_big != ffn.draw_velocities(T, ids, m, kw["seed"] % 2 ** 32, 0)).all()
    # ids NULL: replica 0 of traj_offset = 2^40 + 9 is the replica with that id
    big = dict(dt=kw["dt"], seed=kw["seed"])
    ref = run(eng, pos[2:3], None, T[2:3], ids[2:3], to_nm, **big)
    off = run(eng, pos[2:3], None, T[2:3], None, to_nm, traj_offset=2 ** 40 + 9, **big)
    same(off, ref)
    same([a[2:3] for a in run(eng, pos, None, T, ids, to_nm, **big)], ref)


def test_the_step_index_enters_through_its_low_32_bits():
    """include/ti_hip.h: a run at step_offset = 2^32 + 100 with given velocities is the run at step_offset = 100, bit for bit -- and
    not the run at step_offset = 101"""
    eng, ff, m, pos, T, ids, to_nm, kw = loaded("A9_ids")
    big = dict(dt=kw["dt"], seed=kw["seed"])
    p0, v0, _, _, _ = run(eng, pos, None, T, ids, to_nm, n_steps=0, stride=0, **big)
    low = run(eng, p0, v0, T, ids, to_nm, step_offset=100, **big)
    same(run(eng, p0, v0, T, ids, to_nm, step_offset=2 ** 32 + 100, **big), low)
    other = run(eng, p0, v0, T, ids, to_nm, step_offset=101, **big)
    assert (bits(other[1]) != bits(low[1])).any()
