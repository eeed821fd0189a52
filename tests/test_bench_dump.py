"""bench.py --dump-outputs (no GPU): the array written is float32, whole when it fits DUMP_BYTES and otherwise the
rows a draw from the seed selects — the same rows every time, so two builds' dumps compare row for row."""
import os
import sys

import numpy as np
import torch

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_small_output_is_written_whole(tmp_path):
    bits = torch.from_numpy(np.random.default_rng(0).integers(0, 2, size=(37, 648)).astype(np.uint8))
    bench.dump_outputs(str(tmp_path / "d"), "bits", bits, seed=2024)
    got = np.load(tmp_path / "d" / "bits.npy")
    assert got.dtype == np.float32 and np.array_equal(got, bits.numpy())


def test_large_output_is_a_fixed_seeded_row_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 10 * 4 * 7 + 3)   # room for 10 rows of 7, and a remainder
    bits = torch.arange(25 * 7, dtype=torch.int64).remainder(251).to(torch.uint8).view(25, 7)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), "bits", bits, seed=5)
    a, b = np.load(tmp_path / "a" / "bits.npy"), np.load(tmp_path / "b" / "bits.npy")
    assert a.dtype == np.float32 and a.shape == (10, 7) and np.array_equal(a, b)
    assert a.nbytes <= bench.DUMP_BYTES
    rows = np.sort(np.random.default_rng(5).choice(25, size=10, replace=False))
    assert np.array_equal(a, bits.numpy()[rows])
    bench.dump_outputs(str(tmp_path / "c"), "bits", bits, seed=6)
    assert not np.array_equal(a, np.load(tmp_path / "c" / "bits.npy"))   # the sample follows --seed
    assert os.listdir(tmp_path / "a") == ["bits.npy"]
