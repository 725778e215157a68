"""Scenes with tile lists of prescribed lengths, for the tests of the bucketed key layout (tests/test_gpu_bucket_binning.py).

A camera looks down the world x axis at 128 x 192 pixels (8 x 12 tiles).  Tile (i, 0) of the first tile row holds exactly
`lengths[i]` small splats (radius 4 pixels around the tile centre: one tile each) at shuffled, partly tied depths; a family of
larger splats, centred in tile rows 6-10 and never reaching row 0, touches from a handful to more than 32 tiles each; the last
three Gaussians touch exactly 8, 9 and 72 tiles."""
import functools

import numpy as np

import scenes

H, W = 192, 128
BG = (0.3, 0.1, 0.2)
SH_DEGREE = 1
LENGTHS = (1, 63, 64, 65, 511, 512, 513, 2100)


def camera(azimuth=0.0, elevation=0.0):
    return scenes.camera(elevation, azimuth, 2.0, 40.0, H, W)


def _world(cam, px, py, z):
    """World position of the point at view depth z that projects to pixel (px, py)."""
    nx, ny = (2.0 * px + 1.0) / W - 1.0, (2.0 * py + 1.0) / H - 1.0
    pv = np.stack([nx * z * cam["tanfovx"], ny * z * cam["tanfovy"], z, np.ones_like(z)], -1)
    return (pv @ np.linalg.inv(cam["viewmatrix"].astype(np.float64)))[..., :3]


@functools.lru_cache(maxsize=None)
def list_scene(lengths=LENGTHS, n_big=160, seed=3):
    """Float32 scene arrays (callers do not write to them).  One-tile splats first, list after list, then the large ones."""
    rng = np.random.default_rng(seed)
    cam = camera()
    fx = W / (2.0 * cam["tanfovx"])
    pos, scale, opac = [], [], []
    for i, n in enumerate(lengths):
        z = 2.0 + rng.permutation(n) * 2e-4
        z[1::10] = z[0:-1:10][:len(z[1::10])]                       # ties on depth: the index decides
        px = np.full(n, 16.0 * i + 7.5) + rng.uniform(-1.0, 1.0, n)
        py = np.full(n, 7.5) + rng.uniform(-1.0, 1.0, n)
        pos.append(_world(cam, px, py, z))
        scale.append(np.repeat((1.0 * z / fx)[:, None], 3, 1))      # sigma of one pixel: radius ceil(3 sqrt(1.3)) = 4
        opac.append(rng.uniform(0.006, 0.02, n))
    z = rng.uniform(2.2, 3.0, n_big)
    px, py = rng.uniform(20.0, 108.0, n_big), rng.uniform(110.0, 160.0, n_big)
    pos.append(_world(cam, px, py, z))
    scale.append(rng.uniform(1.0, 25.0, (n_big, 3)) * (z / fx)[:, None])          # radius <= 76 pixels: stays below pixel row 16
    opac.append(rng.uniform(0.05, 0.9, n_big))
    # three round, opaque splats whose tile counts are the same in both list modes: 2 x 4 tiles at the left image border, the
    # 3 x 3 tiles around a tile centre, and 8 x 9 (every tile of their rectangles is reached by the alpha >= 1/255 region)
    fixed = np.array([(2.0, 144.0, 9.0), (71.5, 151.5, 7.0), (64.0, 140.0, 25.0)])         # pixel x, y, sigma in pixels
    z = np.full(len(fixed), 2.5)
    pos.append(_world(cam, fixed[:, 0], fixed[:, 1], z))
    scale.append(np.repeat((fixed[:, 2] * z / fx)[:, None], 3, 1))
    opac.append(np.full(len(fixed), 0.9))
    P = sum(lengths) + n_big + len(fixed)
    q = rng.normal(size=(P, 4))
    q[:sum(lengths)] = (1.0, 0.0, 0.0, 0.0)
    q[-len(fixed):] = (1.0, 0.0, 0.0, 0.0)
    shs = rng.normal(size=(P, (SH_DEGREE + 1) ** 2, 3)) * 0.1
    shs[:, 0, :] = (rng.uniform(0, 1, (P, 3)) - 0.5) / 0.28209479177387814
    return dict(means3D=np.concatenate(pos).astype(np.float32), scales=np.concatenate(scale).astype(np.float32),
                rotations=(q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32),
                opacities=np.concatenate(opac).astype(np.float32)[:, None], shs=shs.astype(np.float32))
