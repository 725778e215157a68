"""Scenes whose tile lists are long (tens of thousands of entries) or walked deep (n_contrib in the thousands), at
64 x 64 pixels: a camera inside a dense ball of large, nearly transparent splats.

  "long"     very long lists (above 16384 entries: the tile sort's beyond-LDS path), walked shallow: every pixel is
             opaque within the first few per cent of its list, the rest of every list lies beyond the tile's deepest
             n_contrib.
  "manyseg"  the same look on 9 x 7 tiles: more than 16384 segments of 64 entries (the backward's persistent grid makes
             a second trip).
  "deep"     lists of 10-17 thousand entries walked to their end; the image stays far from opaque.
  "deeper"   the same with larger splats: 15-24 thousand entries, walked to the end.

tests/test_deep_list_scenes_cpu.py asserts these properties with the CPU oracle alone; tests/test_gpu_deep_lists.py
compares the HIP forward and backward with the oracle on them."""
import functools

import numpy as np

import scenes

BG = (0.3, 0.1, 0.2)
SH_DEGREE = 1
#                 P      H    W    scale factor, opacity range
SCENES = {
    "long":    (90000, 64, 64, 6.0, 0.01, 0.05),
    "deep":    (60000, 64, 64, 1.5, 0.005, 0.012),
    "deeper":  (40000, 64, 64, 3.0, 0.004, 0.008),
    "manyseg": (60000, 144, 112, 5.0, 0.01, 0.05),
}


@functools.lru_cache(maxsize=None)
def _build(name):
    P, H, W, s, lo, hi = SCENES[name]
    rng = np.random.default_rng(5)
    sc = scenes.make_scene("ball", P, seed=5, sh_degree=SH_DEGREE)
    sc["scales"] = (sc["scales"] * s * np.exp(rng.uniform(-0.7, 0.7, (P, 3)))).astype(np.float32)
    q = rng.normal(size=(P, 4))
    sc["rotations"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    sc["opacities"] = rng.uniform(lo, hi, (P, 1)).astype(np.float32)
    return sc


def build(name, azimuth=0.0):
    """(scene dict of float32 arrays, camera, H, W) of the named scene; `azimuth` turns the camera.  The arrays are built
    once and shared by every test that asks for the scene: callers do not write to them."""
    P, H, W = SCENES[name][:3]
    return dict(_build(name)), scenes.camera(0.0, azimuth, 1.2, 40.0, H, W), H, W


def oracle_forward(oracle, name, azimuth=0.0):
    """The oracle's forward of the scene: (RasterOracle with its state, (color, radii, depth, alpha))."""
    sc, cam, H, W = build(name, azimuth)
    ro = oracle.RasterOracle()
    out = ro.forward(image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=np.asarray(BG, np.float32),
                     scale_modifier=1.0, viewmatrix=cam["viewmatrix"], projmatrix=cam["projmatrix"], sh_degree=SH_DEGREE,
                     campos=cam["campos"], means3D=sc["means3D"], opacities=sc["opacities"], shs=sc["shs"],
                     scales=sc["scales"], rotations=sc["rotations"])
    return ro, out


def list_statistics(ro):
    """Per-tile list lengths, the number of 64-entry segments, and per pixel n_contrib and its share of the pixel's list."""
    keys, vals, ranges, tt, nc = ro.binning()
    length = ranges[:, 1].astype(np.int64) - ranges[:, 0].astype(np.int64)
    tiles_x = (ro.W + 15) // 16
    tile_of_pixel = (np.arange(ro.H)[:, None] // 16) * tiles_x + (np.arange(ro.W)[None, :] // 16)
    depth_share = nc / np.maximum(length[tile_of_pixel], 1)
    return dict(lists_min=int(length.min()), lists_median=int(np.median(length)), lists_max=int(length.max()),
                segments=int(((length + 63) // 64).sum()), n_contrib_median=float(np.median(nc)), n_contrib_max=int(nc.max()),
                depth_share_median=float(np.median(depth_share)))
