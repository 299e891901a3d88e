"""bench.py --dump-outputs: what the last timed step computed, written as float32 .npy files within the size budget."""
import os

import numpy as np
import torch


def test_dump_outputs_writes_float32_arrays(tmp_path):
    import bench
    w = torch.randn(30, 20, generator=torch.Generator().manual_seed(1))
    bench.dump_outputs(str(tmp_path), {"loss": torch.tensor([0.25], dtype=torch.float64), "param.w": w})
    assert sorted(os.listdir(tmp_path)) == ["loss.npy", "param.w.npy"]
    loss, pw = np.load(tmp_path / "loss.npy"), np.load(tmp_path / "param.w.npy")
    assert loss.dtype == np.float32 and loss.tolist() == [0.25]
    assert pw.dtype == np.float32 and np.array_equal(pw, w.numpy())


def test_dump_outputs_samples_the_same_elements_when_over_budget(tmp_path):
    import bench
    a = torch.arange(200000, dtype=torch.float32)
    budget = 4096 * 2 + 4 * 50000
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), {"a": a, "b": -a}, budget=budget)
    total = sum(os.path.getsize(tmp_path / "one" / f) for f in os.listdir(tmp_path / "one"))
    assert total <= budget
    x1, x2 = np.load(tmp_path / "one" / "a.npy"), np.load(tmp_path / "two" / "a.npy")
    assert x1.size == 25000 and np.array_equal(x1, x2)
    assert np.all(np.diff(x1) > 0)                            # increasing flat indices of the original array
    assert np.array_equal(np.load(tmp_path / "one" / "b.npy"), -x1)
