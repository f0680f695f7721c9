"""bench.py's output dump (--dump-outputs) and its --full rule, on the CPU."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float32_in_shape(tmp_path):
    import bench
    x = torch.randn(3, 4, 5, dtype=torch.bfloat16)
    got = bench.dump_outputs(str(tmp_path), {"sample": x})
    a = np.load(tmp_path / "sample.npy")
    assert a.dtype == np.float32 and a.shape == (3, 4, 5)
    assert np.array_equal(a, x.float().numpy())
    assert got == {"sample": [[3, 4, 5], 60]}


def test_dump_outputs_samples_a_large_output_within_budget(tmp_path):
    import bench
    x = torch.arange(300_000, dtype=torch.float32).reshape(3, 100_000)
    budget = 256 * 1024
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"sample": x, "other": x[:1, :1000]}, budget=budget)
    files = [tmp_path / d / f for d in ("a", "b") for f in ("sample.npy", "other.npy")]
    assert sum(os.path.getsize(f) for f in files[:2]) <= budget
    a, b = np.load(files[0]), np.load(files[2])
    assert a.dtype == np.float32 and a.ndim == 1 and 0 < a.size < x.numel()
    assert np.array_equal(a, b)                                   # the same seeded sample on every run
    assert np.all(np.diff(a) >= 0) and np.all(np.isin(a, x.numpy()))   # sorted indices into the output itself
    assert np.array_equal(np.load(files[1]), x[:1, :1000].numpy())     # within its share: whole, in its shape


def test_shapes_out_needs_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--shapes-out", "x.txt"], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 2 and "--full" in r.stderr, r.stderr[-2000:]
    assert not os.path.exists(os.path.join(ROOT, "x.txt"))
