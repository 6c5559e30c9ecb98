"""CPU: `bench.py --dump-outputs` writer -- float32 files, whole arrays under the size cap, a fixed seeded sample above it."""
import numpy as np
import torch

from benchlib import dump


def test_small_outputs_are_written_whole(tmp_path):
    x = torch.randn(2, 1, 50, dtype=torch.float32)
    loss = torch.tensor(0.25, dtype=torch.float64)
    dump.dump_outputs(str(tmp_path), {"x": x, "loss": loss})
    got = np.load(tmp_path / "x.npy")
    assert got.dtype == np.float32 and np.array_equal(got, x.numpy())
    assert np.load(tmp_path / "loss.npy").dtype == np.float64


def test_large_outputs_are_a_fixed_sample_under_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(dump, "MAX_BYTES", 4000)
    a = torch.arange(3000, dtype=torch.float32)
    b = torch.arange(1000, dtype=torch.float32).reshape(10, 100)
    for d in ("r1", "r2"):
        dump.dump_outputs(str(tmp_path / d), {"a": a, "b": b}, rank=1, world=2)
    sa, sb = np.load(tmp_path / "r1" / "a.rank1.npy"), np.load(tmp_path / "r1" / "b.rank1.npy")
    assert sa.nbytes + sb.nbytes <= 4000 and sa.size == 750 and sb.size == 250
    assert np.all(np.diff(sa) > 0) and np.isin(sa, a.numpy()).all()          # ascending positions of the original
    assert np.array_equal(sa, np.load(tmp_path / "r2" / "a.rank1.npy"))       # the same sample on every run
