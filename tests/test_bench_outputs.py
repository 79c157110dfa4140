"""bench.dump_outputs on the host: what --dump-outputs writes (float32 .npy files) and the fixed sample it keeps of outputs larger than its
budget."""
import numpy as np
import torch

import bench


def test_dump_outputs_writes_float32_arrays_whole_under_the_budget(tmp_path):
    a, b = torch.arange(12, dtype=torch.float64).reshape(3, 4), torch.ones(5, dtype=torch.bfloat16)
    bench.dump_outputs(str(tmp_path), {"a": a, "b": b})
    ga, gb = np.load(tmp_path / "a.npy"), np.load(tmp_path / "b.npy")
    assert ga.dtype == gb.dtype == np.float32 and ga.shape == (3, 4) and gb.shape == (5,)
    assert np.array_equal(ga, a.float().numpy()) and np.array_equal(gb, np.ones(5, np.float32))


def test_dump_outputs_samples_large_outputs_at_fixed_positions(tmp_path):
    big, small = torch.arange(3000, dtype=torch.float32), torch.arange(1000, dtype=torch.float32) + 0.5
    limit = 1600 + 2 * bench.NPY_HEADER_BYTES                                            # 1600 bytes of data once the two headers are set aside
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small}, max_bytes=limit)
    got = {d: {n: np.load(tmp_path / d / f"{n}.npy") for n in ("big", "small")} for d in ("x", "y")}
    assert got["x"]["big"].size == 300 and got["x"]["small"].size == 100               # the budget shared in proportion to size
    assert sum(f.stat().st_size for f in (tmp_path / "x").iterdir()) <= limit           # the files on disk, headers included
    for n, src in (("big", big), ("small", small)):
        g = got["x"][n]
        assert np.array_equal(g, got["y"][n])                                          # the same positions in every run
        assert np.all(np.diff(g) > 0) and np.isin(g, src.numpy()).all()                 # sorted positions of the flattened output
