"""Seeded inputs of the density-field tests and of tools/make_golden.py group `field` (tests/golden/field.npz).

A cloud shaped like scenes.make_scene("stress", P): a ball of radius 0.5, scales from the 3-NN distance times U(0.3, 3) per axis,
random orientations.  On top of that: one Gaussian in ten has an opacity in (0.001, 0.009), on both sides of the 0.005 prefilter;
eight Gaussians are 1000 times smaller, so that the `+ 1e-24` next to their covariance's determinant (~1e-29) decides their
weight; the quaternions are NOT unit (norms in (0.5, 2)): the field normalises them itself.  Returned raw, as GaussianModel
stores them: opacity before the sigmoid, scaling before the exponential."""
import os

import numpy as np

import scenes

# case -> (P, resolution, num_blocks, seed); c is the default geometry of extract_fields
CASES = {"a": (3000, 32, 8, 21), "b": (3000, 24, 4, 12), "c": (2000, 128, 16, 13)}
C_SAMPLES = 4096
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "field.npz")


def cloud(P, seed):
    """dict(xyz [P, 3], opacity [P, 1] raw, scaling [P, 3] raw, rotation [P, 4] raw), float32."""
    sc = scenes.make_scene("stress", P, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    opac = sc["opacities"].astype(np.float64)
    low = rng.random(P) < 0.1
    opac[low, 0] = rng.uniform(0.001, 0.009, int(low.sum()))
    scales = sc["scales"].astype(np.float64)
    scales[rng.choice(P, 8, replace=False)] *= 1e-3
    rot = sc["rotations"].astype(np.float64) * rng.uniform(0.5, 2.0, (P, 1))
    return dict(xyz=sc["means3D"].astype(np.float32), opacity=np.log(opac / (1 - opac)).astype(np.float32),
                scaling=np.log(scales).astype(np.float32), rotation=rot.astype(np.float32))


def case(name):
    P, R, nb, seed = CASES[name]
    return cloud(P, seed), R, nb


def sample_voxels(R=128, seed=99):
    """The flat voxel indices of case c that the fixture keeps."""
    return np.sort(np.random.default_rng(seed).choice(R ** 3, C_SAMPLES, replace=False))


def load_golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


# ---- edge cases of tests/test_gpu_field.py: name -> (cloud, resolution, num_blocks); same layout as cloud()
def _raw(xyz, opacity, scales, rng):
    P = xyz.shape[0]
    q = rng.normal(size=(P, 4))
    return dict(xyz=xyz.astype(np.float32), opacity=np.log(opacity / (1 - opacity)).reshape(P, 1).astype(np.float32),
                scaling=np.log(scales).astype(np.float32), rotation=q.astype(np.float32))


EDGE_SEEDS = {"single": 40, "transparent": 2, "octant": 41, "packed": 4, "voxel_blocks": 5, "repeat": 6}


def edge_case(name):
    rng = np.random.default_rng(EDGE_SEEDS[name])
    if name == "single":
        return _raw(np.array([[0.2, -0.1, 0.3]]), np.array([0.7]), np.array([[0.5, 0.3, 0.2]]), rng), 32, 8
    if name == "transparent":            # nothing passes the prefilter
        cl = cloud(500, 31)
        o = rng.uniform(0.0005, 0.0049, (500, 1))
        cl["opacity"] = np.log(o / (1 - o)).astype(np.float32)
        return cl, 32, 8
    if name == "octant":                 # one far Gaussian fixes the bounding box; the rest fills one octant of it
        xyz = np.concatenate((rng.uniform(0.1, 0.5, (1500, 3)), [[-0.5, -0.5, -0.5]]))
        return _raw(xyz, rng.uniform(0.05, 0.95, 1501), rng.uniform(0.01, 0.03, (1501, 3)), rng), 32, 8
    if name == "packed":                 # 5000 Gaussians inside block (4, 4, 4), clear of every box face (two anchors fix the bounding
        xyz = np.concatenate((rng.uniform(0.102, 0.124, (5000, 3)), [[-0.5, -0.5, -0.5], [0.5, 0.5, 0.5]]))    # box): a long member list
        return _raw(xyz, rng.uniform(0.05, 0.95, 5002), rng.uniform(0.01, 0.04, (5002, 3)), rng), 32, 8
    if name == "voxel_blocks":           # num_blocks == resolution: one voxel per block
        cl = cloud(500, 32)
        return cl, 16, 16
    if name == "repeat":
        return cloud(1500, 33), 32, 8
    raise ValueError(name)


EDGE_CASES = ("single", "transparent", "octant", "packed", "voxel_blocks")

# ---- blocks of more than 512 voxels: (resolution, num_blocks) -> the seed of cloud(300, seed).  field_eval_kernel holds 1 / 2 / 4 / 8 / 16
# voxels per lane by the block's size and makes a further pass beyond 256 * 16; the cases above stop at 512 voxels per block.  Normalised
# centres lie in [-0.9, 0.9] and the box faces at +-4 (one block) or +-1.47 / +-2.5 (two), so every kept Gaussian is a member of every
# block and no centre is near a face.
LARGE_BLOCK_P = 300
LARGE_BLOCKS = {(10, 1): 51,       # 1000 voxels per block: 4 per lane
                (12, 1): 52,       # 1728: 8 per lane
                (16, 1): 53,       # 4096: 16 per lane, exactly one pass
                (17, 1): 54,       # 4913: 16 per lane, two passes, a ragged tail of 817
                (34, 2): 55}       # 4913 in each of 8 blocks: the same with non-zero block coordinates


def large_block_case(R, nb):
    return cloud(LARGE_BLOCK_P, LARGE_BLOCKS[(R, nb)]), R, nb
