"""bench.py --dump-outputs (no GPU needed): the packed x^ words a caller of Decoder.decode()
receives come back as float32 bits, whole for a small batch and as the same seeded, sorted
sample of frames on every run for a batch above the size limit."""
import numpy as np
import torch

import bench


def test_dump_outputs_whole_and_sampled(pkg, tmp_path, monkeypatch):
    N, B = 128, 37
    bits = np.random.default_rng(5).integers(0, 2, size=(B, N)).astype(np.uint8)
    out = torch.from_numpy(pkg.pack_bits(bits).view(np.int64))
    path = tmp_path / "dump" / "xhat.npy"
    bench.dump_outputs(torch, pkg, out, N, str(path))
    a = np.load(path)
    assert a.dtype == np.float32 and a.shape == (B, N) and (a == bits).all()
    # a limit of 10 frames: 10 distinct frames in batch order, the same ones on every run
    monkeypatch.setattr(bench, "DUMP_BYTES", 10 * 4 * N)
    bench.dump_outputs(torch, pkg, out, N, str(path))
    s = np.load(path)
    assert s.dtype == np.float32 and s.shape == (10, N)
    rows = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(B, 10, replace=False))
    assert len(set(rows.tolist())) == 10 and (s == bits[rows]).all()
    bench.dump_outputs(torch, pkg, out, N, str(tmp_path / "again.npy"))
    assert (np.load(tmp_path / "again.npy") == s).all()
