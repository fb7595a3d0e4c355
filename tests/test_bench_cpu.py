"""bench.py --dump-outputs, host side: float32 .npy files, under 64 MB in all, the same seeded rows on every call."""
import numpy as np
import torch

import bench


def test_dump_outputs_writes_a_small_output_whole_as_float32(tmp_path):
    y = torch.randn(8, 16).half()
    bench.dump_outputs(str(tmp_path), {"y": y})
    a = np.load(tmp_path / "y.npy")
    assert a.dtype == np.float32 and np.array_equal(a, y.float().numpy())


def test_dump_outputs_samples_the_same_whole_rows_of_a_large_output_under_64_mb(tmp_path):
    M, N = 8192, 4096                                                # 128 MiB as float32
    y = torch.arange(M, dtype=torch.float32)[:, None].expand(M, N)   # every element holds its row index
    bench.dump_outputs(str(tmp_path / "a"), {"y": y})
    bench.dump_outputs(str(tmp_path / "b"), {"y": y})
    assert (tmp_path / "a" / "y.npy").stat().st_size <= 64e6
    a, b = np.load(tmp_path / "a" / "y.npy"), np.load(tmp_path / "b" / "y.npy")
    assert a.dtype == np.float32 and a.shape[1] == N and 0 < a.shape[0] < M
    assert np.array_equal(a, b)
    rows = a[:, 0]
    assert np.array_equal(a, np.broadcast_to(rows[:, None], a.shape))    # whole rows, not scattered elements
    assert np.all(np.diff(rows) > 0)                                      # each row once, in order
