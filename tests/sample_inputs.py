"""Seeded inputs of the field-sampler tests (tests/test_gpu_sample.py), next to the clouds of tests/field_inputs.py.  Clouds are
returned raw, as GaussianModel stores them: opacity before the sigmoid, scaling before the exponential."""
import math

import numpy as np
import torch

import sample_reference

ONE_PASS = 1024          # points one pass of the evaluate kernel holds: 256 lanes * SAMPLE_PPT (csrc/field_sample.hip)


def grid_points(R):
    """Every grid point of an R^3 grid as float32 grid values, [R^3, 3] in `ij` order: point (i, j, k) is row (i * R + j) * R + k."""
    g = torch.linspace(-1, 1, R, dtype=torch.float32)
    return torch.stack(torch.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).contiguous()


def colors(P, seed):
    return np.random.default_rng(seed).uniform(0, 1, (P, 3)).astype(np.float32)


def offgrid_points(R, nb, seed=7):
    """About 6000 normalised float32 points in [-1.1, 1.1]^3 (so some lie outside the grid) and their blocks, arranged so that one
    block holds more points than one pass of the kernel, the last block holds none and block (0, 0, nb - 1) holds exactly one.
    Shuffled: the caller's order is not the blocks' order."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(-1.1, 1.1, (4500, 3)).astype(np.float32)
    blk = sample_reference.point_blocks(u, R, nb)
    none, one = nb ** 3 - 1, nb - 1
    u = u[(blk != none) & (blk != one)]
    grid = torch.linspace(-1, 1, R, dtype=torch.float32).numpy()
    s = R // nb
    # the crowded block (1, nb - 2, 1): uniform between its first grid value and the next block's first
    lo = np.array([grid[s], grid[(nb - 2) * s], grid[s]], np.float64)
    hi = np.array([grid[2 * s], grid[(nb - 1) * s], grid[2 * s]], np.float64)
    crowd = (lo + (hi - lo) * rng.uniform(0.01, 0.99, (1500, 3))).astype(np.float32)
    single = np.array([[-0.9, -0.8, 0.95]], np.float32)
    u = np.concatenate((u, crowd, single))
    u = np.ascontiguousarray(u[rng.permutation(len(u))])
    blk = sample_reference.point_blocks(u, R, nb)
    counts = np.bincount(blk, minlength=nb ** 3)
    assert counts.max() > ONE_PASS and counts[none] == 0 and counts[one] == 1, (counts.max(), counts[none], counts[one])
    return u, blk


# ---- one isotropic Gaussian between two small far ones that fix the extent (scale = 1.8 / 1.0, center = 0)
SPHERE_MU = np.array([0.1, -0.05, 0.2])
SPHERE_SIGMA, SPHERE_OPACITY, SPHERE_THRESHOLD = 0.15, 0.9, 0.5
SPHERE_COLOR = (0.2, 0.5, 0.8)
FAR_XYZ = np.array([[-0.5, -0.5, -0.5], [0.5, 0.5, 0.5]])
FAR_SIGMA, FAR_OPACITY = 0.03, 0.3      # FAR_OPACITY < SPHERE_THRESHOLD: below the threshold everywhere
SPHERE_RADIUS = SPHERE_SIGMA * math.sqrt(2 * math.log(SPHERE_OPACITY / SPHERE_THRESHOLD))


def sphere_cloud():
    """(cloud, colors [3, 3]): the Gaussian of the sphere first."""
    xyz = np.concatenate((SPHERE_MU[None], FAR_XYZ)).astype(np.float32)
    opac = np.array([SPHERE_OPACITY, FAR_OPACITY, FAR_OPACITY])
    sig = np.array([[SPHERE_SIGMA] * 3, [FAR_SIGMA] * 3, [FAR_SIGMA] * 3])
    rot = np.zeros((3, 4), np.float32)
    rot[:, 0] = 1
    cl = dict(xyz=xyz, opacity=np.log(opac / (1 - opac)).reshape(3, 1).astype(np.float32), scaling=np.log(sig).astype(np.float32),
              rotation=rot)
    return cl, np.array([SPHERE_COLOR, (1.0, 0.0, 0.0), (0.0, 1.0, 0.0)], np.float32)


def blob_cloud(P=3000, seed=17):
    """P Gaussians uniform in a ball of radius 0.5, sigma in (0.03, 0.05) per axis, random orientations, opacity in (0.4, 0.8): the
    density inside is about 3.5, so density 1 is a closed surface near the ball's; sigma is over two grid spacings at R 64."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(P, 3))
    xyz = 0.5 * d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0, 1, (P, 1)) ** (1 / 3)
    opac = rng.uniform(0.4, 0.8, (P, 1))
    return dict(xyz=xyz.astype(np.float32), opacity=np.log(opac / (1 - opac)).astype(np.float32),
                scaling=np.log(rng.uniform(0.03, 0.05, (P, 3))).astype(np.float32), rotation=rng.normal(size=(P, 4)).astype(np.float32))
