"""bench.py --dump-outputs on the CPU: what dump_outputs writes for the headline step's arrays (float32, a fixed sample of the large
ones, under 64 MB in all), and the --steps check of the command line."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _headline_arrays(V=4, P=100000, H=1024, W=1024):
    """Tensors of the shapes and dtypes the timed step returns at the default arguments, with distinct entries."""
    g = torch.Generator().manual_seed(0)
    return {"color": torch.rand(V, 3, H, W, generator=g), "radii": torch.randint(0, 50, (V, P), dtype=torch.int32, generator=g),
            "depth": torch.rand(V, 1, H, W, generator=g), "alpha": torch.rand(V, 1, H, W, generator=g),
            "grad_means3D": torch.randn(P, 3, generator=g), "grad_shs": torch.randn(P, 1, 3, generator=g),
            "grad_opacities": torch.randn(P, 1, generator=g), "grad_scales": torch.randn(P, 3, generator=g),
            "grad_rotations": torch.randn(P, 4, generator=g), "grad_means2D": torch.randn(V, P, 3, generator=g)}


def test_dump_writes_float32_and_a_fixed_sample_under_64_mb(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    arrays = _headline_arrays()
    info = bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    assert sorted(os.listdir(tmp_path / "a")) == sorted(n + ".npy" for n in arrays)
    total = 0
    for name, t in arrays.items():
        a = np.load(tmp_path / "a" / (name + ".npy"))
        assert a.dtype == np.float32 and info[name]["shape"] == list(t.shape) and info[name]["written"] == a.size
        full = t.float().numpy()
        if full.size <= bench.DUMP_MAX_ELEMENTS:
            assert np.array_equal(a, full)                                       # small arrays: whole, shape kept
        else:
            assert a.shape == (bench.DUMP_MAX_ELEMENTS,)
            idx = np.sort(np.random.default_rng(0).choice(full.size, bench.DUMP_MAX_ELEMENTS, replace=False))
            assert np.array_equal(a, full.reshape(-1)[idx])                      # the documented entries, in index order
        assert np.array_equal(a, np.load(tmp_path / "b" / (name + ".npy")))      # the same sample in every run
        total += os.path.getsize(tmp_path / "a" / (name + ".npy"))
    assert total <= 64 * 2 ** 20


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr and r.stdout == ""
