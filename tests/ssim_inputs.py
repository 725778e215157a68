"""Inputs of the SSIM fixtures (tests/golden/ssim*.npz), regenerated from numpy seeds: shared by tools/make_golden.py (group
`ssim`) and by the tests, so the golden files hold the reference's OUTPUTS only.

A case is (kind, shape); `images(kind, shape)` returns (img1, img2) float32 [N, C, H, W] in [0, 1]."""
import glob
import os
import zlib

import numpy as np

KINDS = ("rand", "smooth", "near", "flat", "dark", "same")
# the kernel's tile is 32 x 32
SHAPES = (
    (1, 1, 7, 9),       # smaller than the window in both directions: all padding
    (1, 3, 11, 11),     # exactly the window
    (2, 3, 45, 67),     # partial tiles in both directions, batch and channel strides
    (1, 4, 32, 32),     # exactly one tile, 4 channels
    (1, 1, 33, 65),     # one pixel past a tile edge
    (2, 3, 96, 80),     # several whole tiles
)
CASES = tuple((k, s) for k in KINDS for s in SHAPES)
STAGE3_CASE = ("smooth", (4, 3, 415, 290))      # the stage-3 crop at half resolution; its golden entry holds error figures, no gradient
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def case_key(kind, shape):
    return "%s_%s" % (kind, "x".join(str(d) for d in shape))


def _box9(a):
    """9 x 9 box filter with edge replication, per plane."""
    H, W = a.shape[-2:]
    p = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(4, 4), (4, 4)], mode="edge")
    out = np.zeros_like(a)
    for dy in range(9):
        for dx in range(9):
            out += p[..., dy:dy + H, dx:dx + W]
    return out / 81.0


def images(kind, shape):
    rng = np.random.default_rng(zlib.crc32(case_key(kind, shape).encode()))
    N, C, H, W = shape
    if kind == "rand":
        a, b = rng.random(shape), rng.random(shape)
    elif kind == "smooth":       # render-like: the largest cancellation in E[x^2] - mu^2
        a = _box9(rng.random(shape))
        b = np.clip(a + 0.05 * (rng.random(shape) - 0.5), 0.0, 1.0)
    elif kind == "near":
        a = rng.random(shape)
        b = np.clip(a + 0.02 * (rng.random(shape) - 0.5), 0.0, 1.0)
    elif kind == "flat":         # a constant against a constant with a step edge
        a = np.full(shape, 0.7)
        b = np.full(shape, 0.7)
        b[..., :, W // 2:] = 0.4
    elif kind == "dark":
        a, b = 0.02 * rng.random(shape), 0.02 * rng.random(shape)
    elif kind == "same":
        a = rng.random(shape)
        b = a
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)


def load_golden():
    """All arrays of tests/golden/ssim*.npz in one dict: `<case>_scalar`, `<case>_vector` [N], `<case>_grad` [N, C, H, W] (those of
    the largest shape live in ssim_grad_*.npz: no file above 1 MiB), `<case>_map_err` (the reference's float32 map against its
    float64 map, maximum); STAGE3_CASE has `_grad_err` (the same for its gradient, over max|grad|) instead of `_grad`."""
    out = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN_DIR, "ssim*.npz"))):
        with np.load(path) as d:
            for k in d.files:
                out[k] = d[k]
    return out
