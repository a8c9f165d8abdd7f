"""bench.py --dump-outputs, on the CPU: float32 .npy files, whole arrays while they fit, and past the 64 MB budget a seeded
sample of trajectories that is the same from run to run."""
import os

import numpy as np

import bench


def _dump(d, arrays):
    bench.dump_outputs(str(d), arrays)
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_small_outputs_are_written_whole(tmp_path):
    a = np.random.default_rng(1).standard_normal((100, 18, 3))
    got = _dump(tmp_path, {"end_states": a, "f32_mfma_path_end_states": a[:10]})
    assert set(got) == {"end_states", "f32_mfma_path_end_states"}
    assert got["end_states"].dtype == np.float32 and np.array_equal(got["end_states"], a.astype(np.float32))
    assert np.array_equal(got["f32_mfma_path_end_states"], a[:10].astype(np.float32))


def test_large_outputs_are_a_fixed_sample_within_the_budget(tmp_path):
    a = np.arange(8 * 65536, dtype=np.float32)[:, None, None] * np.ones((1, 18, 3), np.float32)     # row i holds i
    arrays = {"end_states": a, "f32_mfma_path_end_states": a[:65536]}
    first, second = _dump(tmp_path / "a", arrays), _dump(tmp_path / "b", arrays)
    total = sum(os.path.getsize(os.path.join(tmp_path / "a", f)) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_BYTES
    rows = first["end_states"][:, 0, 0]
    assert 0 < len(rows) < a.shape[0] and np.all(np.diff(rows) > 0)                 # distinct rows, ascending
    assert np.array_equal(first["end_states"], a[rows.astype(np.int64)])
    assert np.array_equal(first["end_states"], second["end_states"])                # same sample every run
    assert np.array_equal(first["f32_mfma_path_end_states"], a[:65536])             # 14 MB fits its share whole
