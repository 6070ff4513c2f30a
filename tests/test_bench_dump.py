"""bench.py --dump-outputs on the host (no GPU): exact values, the byte cap, the seeded row sample of an output too large to
write whole, and the padding of rows that hold fewer entries than their width."""
import os

import numpy as np
import torch

import bench


def test_dump_outputs_cap_sample_and_padding(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 20)
    rng = np.random.default_rng(5)
    n, width = 1000, 600
    scores = torch.from_numpy(rng.integers(-5, 1 << 20, n).astype(np.int32))
    lengths = torch.from_numpy(rng.integers(1, width + 1, n).astype(np.int32))
    tb = torch.from_numpy(rng.integers(0, 16384, (n, width, 2)).astype(np.int32))
    outputs = [("scores", scores), ("traceback_lengths", lengths), ("tracebacks", tb, lengths)]
    for d in ("a", "b"):
        bench.dump_outputs(np, torch, str(tmp_path / d), outputs)

    got = {f[:-4]: np.load(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))}
    assert sorted(got) == ["scores", "traceback_lengths", "tracebacks"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 1 << 20
    assert np.array_equal(got["scores"], scores.numpy()) and np.array_equal(got["traceback_lengths"], lengths.numpy())
    kept = got["tracebacks"]
    assert 0 < kept.shape[0] < n and kept.shape[1:] == (width, 2)
    rows = np.sort(np.random.default_rng(bench.DUMP_SAMPLE_SEED).choice(n, kept.shape[0], replace=False))
    for k, r in enumerate(rows):
        ln = int(lengths[r])
        assert np.array_equal(kept[k, :ln], tb[r, :ln].numpy()) and (kept[k, ln:] == -1).all()
    for name, a in got.items():                      # the same arguments write the same files
        assert np.array_equal(a, np.load(str(tmp_path / "b" / (name + ".npy"))))
