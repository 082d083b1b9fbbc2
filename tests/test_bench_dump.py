"""CPU: bench.py --dump-outputs writes the timed step's outputs, capped in size by a fixed sample of envs."""
import os

import numpy as np

import bench


def _outputs(n):
    return {"state": np.arange(n * 20, dtype=np.float64).reshape(n, 20), "reward": np.arange(n, dtype=np.float64),
            "done": (np.arange(n) % 3 == 0).astype(np.float32)}


def test_dump_writes_every_array_whole(tmp_path):
    outs = _outputs(4096)
    info = bench.dump_outputs(str(tmp_path), outs)
    assert info["sampled_envs"] is None
    assert sorted(os.listdir(str(tmp_path))) == ["done.npy", "reward.npy", "state.npy"]
    for name, a in outs.items():
        b = np.load(str(tmp_path / (name + ".npy")))
        assert b.dtype == a.dtype and np.array_equal(a, b)


def test_dump_above_the_limit_is_a_fixed_sample_of_rows(tmp_path):
    n = 400000                                  # 400 000 x 172 B > 64 MB
    outs = _outputs(n)
    bench.dump_outputs(str(tmp_path / "a"), outs)
    bench.dump_outputs(str(tmp_path / "b"), outs)
    total = sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a")))
    assert total <= bench.DUMP_LIMIT_BYTES
    ids = np.load(str(tmp_path / "a" / "env_ids.npy"))
    assert ids.dtype == np.float64 and len(ids) > n // 2 and np.all(np.diff(ids) > 0)
    rows = ids.astype(np.int64)
    for name, a in outs.items():
        got = np.load(str(tmp_path / "a" / (name + ".npy")))
        assert np.array_equal(got, a[rows])
        assert np.array_equal(got, np.load(str(tmp_path / "b" / (name + ".npy"))))
