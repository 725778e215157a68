"""Seeded meshes of the texture-baking tests (tests/test_texture_cpu.py, tests/test_gpu_texture.py).  Vertices are float32 in the
field's NORMALISED coordinates unless said otherwise; every triangle has three vertices of its own."""
import numpy as np
import torch

import sample_inputs
import sample_reference
import texture_reference

ONE_PASS = 1024          # texel slots one pass of the bake kernel holds: 256 lanes * TEX_PPT (csrc/texture.hip)
PARITY_SIZE = 128


def slots_per_face(c):
    """Texel slots the kernel enumerates per face (csrc/texture.hip): c (c + 1) / 2, of which an odd face skips c."""
    return c * (c + 1) // 2


def _triangles(centres, half_extent, rng):
    return (centres[:, None, :] + rng.uniform(-half_extent, half_extent, (len(centres), 3, 3))).astype(np.float32)


def _blocks(tri, R, nb):
    cen = (tri[:, 0] + tri[:, 1] + tri[:, 2]) / np.float32(3)
    return sample_reference.point_blocks(cen, R, nb)


def parity_mesh(R, nb, seed=23):
    """(vertices [3 F, 3], faces [F, 3] int32), about 600 faces: 300 small triangles (half-extent 0.04) with centres uniform in
    [-1.05, 1.05]^3, so some lie outside the grid, none with its centroid in the last block or in block (0, 0, nb - 1); 300 (half-extent
    0.02) inside block (1, nb - 2, 1); one face alone in block (0, 0, nb - 1), at (-0.9, -0.8, 0.95); one degenerate face, three equal
    vertices.  Shuffled.  Also returns the index of the degenerate face."""
    rng = np.random.default_rng(seed)
    wide = _triangles(rng.uniform(-1.05, 1.05, (300, 3)), 0.04, rng)
    none, one = nb ** 3 - 1, nb - 1
    blk = _blocks(wide, R, nb)
    wide = wide[(blk != none) & (blk != one)]
    grid = torch.linspace(-1, 1, R, dtype=torch.float32).numpy().astype(np.float64)
    s = R // nb
    lo = np.array([grid[s], grid[(nb - 2) * s], grid[s]])
    hi = np.array([grid[2 * s], grid[(nb - 1) * s], grid[2 * s]])
    crowd = _triangles(lo + (hi - lo) * rng.uniform(0.1, 0.9, (300, 3)), 0.02, rng)
    single = _triangles(np.array([[-0.9, -0.8, 0.95]]), 0.02, rng)
    flat = np.repeat(np.array([[[0.3, 0.2, -0.4]]], np.float32), 3, axis=1)
    tri = np.concatenate((wide, crowd, single, flat))
    perm = rng.permutation(len(tri))
    tri = np.ascontiguousarray(tri[perm])
    degenerate = int(np.nonzero(perm == len(tri) - 1)[0][0])
    blk = _blocks(tri, R, nb)
    counts = np.bincount(blk, minlength=nb ** 3)
    crowded = (1 * nb + (nb - 2)) * nb + 1
    assert counts[none] == 0 and counts[one] == 1 and counts[crowded] >= 300 and counts.argmax() == crowded, counts
    assert (np.abs(tri) > 1).any()
    F = len(tri)
    return tri.reshape(-1, 3), np.arange(3 * F, dtype=np.int32).reshape(F, 3), degenerate


def random_mesh(F, seed, extent=0.6, half_extent=0.05):
    """(vertices [3 F, 3], faces [F, 3] int32): F seeded triangles with centres in [-extent, extent]^3."""
    rng = np.random.default_rng(seed)
    tri = _triangles(rng.uniform(-extent, extent, (F, 3)), half_extent, rng)
    return tri.reshape(-1, 3), np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def sphere_mesh(F=40, seed=3):
    """F small triangles (world coordinates, float32) around points of the sphere density == SPHERE_THRESHOLD of
    sample_inputs.sphere_cloud, where the two far Gaussians weigh nothing."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(F, 3))
    centres = sample_inputs.SPHERE_MU + sample_inputs.SPHERE_RADIUS * d / np.linalg.norm(d, axis=1, keepdims=True)
    tri = _triangles(centres, 0.03, rng)
    return tri.reshape(-1, 3), np.arange(3 * F, dtype=np.int32).reshape(F, 3)


def face_samples(uv):
    """[F, 7, 2] float64: every face's three corners, three edge midpoints and barycentre in OBJ texture coordinates."""
    t = np.asarray(uv, np.float64)
    mid = (t + np.roll(t, -1, axis=1)) / 2
    return np.concatenate((t, mid, t.mean(1, keepdims=True)), 1)


def layout_cases():
    return [(1, 8), (2, 8), (7, 16), (50, 32), (1000, 128), (131072, 1024)]

