"""bench.py's --dump-outputs writer on the host: whole output below the budget, a fixed seeded sample of whole rows
above it, float32 / float64 files only, within the budget."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_small_output_is_written_whole(tmp_path):
    out = torch.randn(100, 40)
    bench.dump_outputs(out, str(tmp_path), 0, 1, 1234)
    assert sorted(os.listdir(tmp_path)) == ["out.npy"]
    got = np.load(tmp_path / "out.npy")
    assert got.dtype == np.float32 and np.array_equal(got, out.numpy())


def test_large_output_is_a_seeded_sample_of_rows(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 20_000)
    out = torch.randn(1000, 48)
    for rank, sub in ((0, "a"), (0, "b"), (1, "c")):
        bench.dump_outputs(out, str(tmp_path / sub), rank, 2, 1234)
    assert sorted(os.listdir(tmp_path / "c")) == ["out_rank1.npy", "out_rank1_rows.npy"]
    rows = np.load(tmp_path / "a" / "out_rank0_rows.npy")
    got = np.load(tmp_path / "a" / "out_rank0.npy")
    assert rows.dtype == np.float64 and got.dtype == np.float32
    assert rows.size == 10_000 // (48 * 4 + 8) and (np.diff(rows) > 0).all()
    assert np.array_equal(got, out.numpy()[rows.astype(np.int64)])
    assert got.nbytes + rows.nbytes <= 10_000
    assert np.array_equal(rows, np.load(tmp_path / "b" / "out_rank0_rows.npy"))       # same seed, same sample
