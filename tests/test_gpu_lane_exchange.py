"""The backward blend's cross-lane fold exchanges half-waves over the LDS crossbar (csrc/bwd_fold.h: fold_two_entries,
ds_bpermute_b32 at lane ^ 32 and ds_swizzle_b32 at lane ^ 16) where it used v_permlane32/16_swap.  The crossbar network
feeds the same operand pairs into the same adds, so it must leave the same bits.

`tools/micro/fold_check.hip` is a stand-alone program that includes the header, runs the swap network (kept there for
this purpose, launched by nothing in the library) and the crossbar network on the same 4096 accumulator sets of 20 registers
x 64 lanes and compares all twenty sums of every set in the lanes the row store reads: normal values, magnitudes mixed from
1e-30 to 1e30, +-0 / denormals / infinities, and an all-zero entry B (the odd tail of a list).  Equal bits, NaNs in the
same places; it also ties one set to the plain sum in float64 and refuses a fold that leaves zeros everywhere.  It exits
non-zero on the first difference.  The test builds it for gfx950 and runs it as a child process under a time limit.

The forward blend exchanges a pair's two alphas, the checkpoints' half sums and the epilogue's half sums between the
lane halves (csrc/render_forward.hip: both32, xchg32).  It still does so with v_permlane32_swap: the crossbar form of that
exchange measured slower and was not adopted (tools/experiments/render_forward_crossbar.diff.txt), so the forward tests
below cover no change of this kernel; they pin the shapes at which any other form of the exchange would have to hold, for
the next attempt.  Smallest shapes at which the exchange can go wrong, sh_degree 0:
  * one 16 x 16 tile (a 16 x 16 image) with 1, 2, 3 and 5 live entries, each wide enough to be live in all eight 8 x 4
    blocks of the tile, so every wave walks them all and the second entry of the last pair of an odd count is the NULL slot;
  * one tile with 65 and one with 129 such entries: the walk crosses one / two 64-entry segment boundaries and writes a
    checkpoint there from the two lane halves' partial sums; the backward reads it back, so these two scenes are also held
    to the oracle's gradients;
  * a 20 x 20 image: four tiles, three of them partial edge tiles.
The oracle's lists and a float64 alpha test assert these counts on the CPU, and that no threshold test of any pixel sits on
a knife edge (so n_contrib must equal the oracle's at every pixel), before anything runs on the GPU.  Then: images against
the oracle at test_gpu_raster_parity's bars (IMG_TOL, BACKWARD_TOL, unchanged), and two runs with equal bits."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from test_gpu_bwd_pair_fold import _alpha_region, _camera, _gaussians
from test_gpu_raster_parity import KNIFE_EDGE, _check_backward, _check_forward_scene, _dev, _oracle_forward, _settings

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_crossbar_network_equals_swap_network_bit_for_bit(tmp_path):
    exe = str(tmp_path / "fold_check")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-I", os.path.join(ROOT, "gaussianip_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tools", "micro", "fold_check.hip")], check=True, capture_output=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads(r.stdout.strip().splitlines()[0])
    assert res["fold_check"] == "equal" and res["network"] == "crossbar" and res["against"] == "swap" and res["sets"] == 4096
    assert res["sums_compared"] == 4096 * 20
    assert res["nan_sums"] > 0, "the infinities of class 2 must have met (NaN positions are part of the comparison)"


BG = (0.3, 0.1, 0.2)
# name -> (image side, Gaussians, seed); the seeds are the first whose scene has no knife-edge pixel (asserted below)
FORWARD_SCENES = {"1": (16, 1, 0), "2": (16, 2, 0), "3": (16, 3, 0), "5": (16, 5, 0), "65": (16, 65, 0), "129": (16, 129, 0),
                  "20x20": (20, 40, 0)}


@functools.lru_cache(maxsize=None)
def _scene(name):
    """One tile: centres on pixel corners within 2 pixels of the tile's middle, axes 12-28 pixels, so that even at opacity 0.03 the alpha
    at the tile's farthest corner, 13.4 pixels away, is four times 1/255 (no alpha near the threshold: 129 entries x 256
    pixels would otherwise put a few within KNIFE_EDGE of it); opacity at most 0.3, about 5 / n (T stays above 5e-3: no pixel
    terminates).  20 x 20: centres anywhere in the image, 1.5-3 pixels wide.
    All depths distinct."""
    side, n, seed = FORWARD_SCENES[name]
    rng = np.random.default_rng(1000 * n + seed)
    cam = _camera(side, side)
    lo, hi, smin, smax = (6.5, 9.5, 20.0, 28.0) if side == 16 else (1.0, 19.0, 1.5, 3.0)
    px, py = rng.uniform(lo, hi, n), rng.uniform(lo, hi, n)
    if side == 16:      # on pixel corners: so wide a Gaussian has |power| < KNIFE_EDGE within a fifth of a pixel of its centre
        px, py = np.floor(px) + 0.5, np.floor(py) + 0.5
    z = 2.0 + 0.002 * rng.permutation(n)
    opacity = rng.uniform(0.8, 1.0, n) * min(0.3, (5.0 if side == 16 else 8.0) / n)
    return _gaussians(rng, cam, side, side, px, py, z, rng.uniform(smin, smax, n), opacity, 0), cam, side


def _assert_on_cpu(oracle, name):
    """List lengths, live entries per 8 x 4 block of tile 0, no terminated pixel, no knife edge.  Returns n_contrib."""
    sc, cam, side = _scene(name)
    n = FORWARD_SCENES[name][1]
    ro, _ = _oracle_forward(oracle, sc, cam, side, side, BG, 0)
    keys, vals, ranges, tt, nc = ro.binning()
    geom = ro.geom()
    ids = vals[int(ranges[0, 0]):int(ranges[0, 1])].astype(np.int64)
    if side == 16:
        assert ranges.shape[0] == 1 and ids.shape[0] == n, (ranges.shape, ids.shape)
        live = np.stack([_alpha_region(geom, g, 0, 0, 16, 16) for g in ids])            # [entry, y, x]
        per_block = [int(live[:, (b >> 1) * 4:(b >> 1) * 4 + 4, (b & 1) * 8:(b & 1) * 8 + 8].any((1, 2)).sum()) for b in range(8)]
        assert per_block == [n] * 8, per_block      # every wave walks every entry, across every segment boundary
        assert int(nc.max()) == n and int(nc.min()) > 64 * ((n - 1) // 64), "no pixel terminates in front of the last segment"
    else:
        assert ranges.shape[0] == 4 and all(int(ranges[t, 1]) - int(ranges[t, 0]) >= 5 for t in range(4)), ranges
    assert float(ro.pixel_margins(np.arange(side * side)).min()) >= KNIFE_EDGE, "a knife-edge pixel: pick another seed"
    return nc


def _forward(name):
    from gaussianip_amd import rasterizer as R
    sc, cam, side = _scene(name)
    (color, radii, depth, alpha), plan = R.forward_with_state(
        _dev(sc["means3D"]), _dev(sc["opacities"]), [_settings(cam, side, side, BG, 0)], shs=_dev(sc["shs"]), scales=_dev(sc["scales"]),
        rotations=_dev(sc["rotations"]))
    torch.cuda.synchronize()
    return color[0].clone(), depth[0].clone(), alpha[0].clone(), R.state_views(plan)["n_contrib"][0].clone()


@pytest.mark.parametrize("name", list(FORWARD_SCENES))
def test_forward_pair_exchange_at_the_smallest_shapes(oracle, name):
    sc, cam, side = _scene(name)
    nc = _assert_on_cpu(oracle, name)
    _check_forward_scene(oracle, sc, cam, side, side, 0, bg=BG, nc_mismatch_frac=0.0)     # images at IMG_TOL, n_contrib equal everywhere
    a, b = _forward(name), _forward(name)
    for what, x, y in zip(("color", "depth", "alpha", "n_contrib"), a, b):
        assert torch.equal(x, y) and float(x.float().abs().max()) > 0.0, what
    assert int(a[3].max()) > 0 and int(nc.max()) > 0


@pytest.mark.parametrize("name", ["65", "129"])
def test_checkpoint_half_sums_reach_the_backward(oracle, name):
    """The checkpoint at a segment boundary is the sum of the two lane halves' partial sums; the backward starts the next
    segment from it.  Gradients against the oracle at BACKWARD_TOL."""
    sc, cam, side = _scene(name)
    _assert_on_cpu(oracle, name)
    _check_backward(oracle, "lane exchange " + name, FORWARD_SCENES[name][1], side, side, 7, 0, scene=dict(sc), cam=cam, bg=BG)
