"""The seeded inputs of the marching-tetrahedra tests on the reference's 32-grid (tests/golden/tets_32.npz: 5034 vertices on [0, 1]^3,
24 444 tetrahedra; tests/golden/isosurface.npz holds the reference's values on them; pure numpy).

case(name) -> (sdf [Nv, 1] float32, deformation [Nv, 3] float32 or None):
  "sphere"  |x - 0.5| - 0.3, no deformation.
  "noise"   inside the ball |x - 0.5| < NOISE_RADIUS a random sign times a magnitude uniform in [0.25, 1], outside it the magnitude alone
            (positive: unoccupied space has one sign, so the surface stays inside the ball and the fixture small), with a deformation
            of 0.3 * standard normal, which the helper bounds by tanh / resolution.  The magnitude's floor keeps the denominator of
            every crossing edge at |d| >= 0.5, so the 1 / d^2 of the distance's gradient cannot blow a comparison up.
  "zeros"   the sphere with the distance set to exactly 0 on a seeded tenth of the vertices: `> 0` (marching tetrahedra) and `sign`
            (tet_sdf_diff) treat a zero differently.
weights(name, V) -> w [V, 3] float32: the seeded weight of the vertices' gradient, d(sum w . v_pos).
All arithmetic is float64 in a written order and rounded to float32 once, so the arrays do not depend on numpy's summation."""
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TETS = os.path.join(HERE, "golden", "tets_32.npz")
GOLDEN = os.path.join(HERE, "golden", "isosurface.npz")
RESOLUTION = 32
CASES = ("sphere", "noise", "zeros")
SEEDS = {"sphere": 21, "noise": 22, "zeros": 23}
NOISE_RADIUS = 0.36
MIN_CASE_COUNT = 50
# per case: the quantities of the fixture with a float32 error of the reference ("def": the deformation, "pos": the grid positions)
QUANTITIES = {"sphere": ("v_pos", "g_sdf", "g_pos", "tsd", "g_tsd"), "noise": ("v_pos", "g_sdf", "g_def", "tsd", "g_tsd"),
              "zeros": ("v_pos", "g_sdf", "g_pos", "tsd", "g_tsd")}


@functools.lru_cache(maxsize=None)
def _grid():
    with np.load(TETS) as z:
        return z["vertices"].astype(np.float32), z["indices"].astype(np.int64)


def grid():
    """(vertices [5034, 3] float32, indices [24444, 4] int64) of the 32-grid, as the reference's helper holds them."""
    v, t = _grid()
    return v.copy(), t.copy()


def _radius(v):
    c = v.astype(np.float64) - 0.5
    return np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])


@functools.lru_cache(maxsize=None)
def _case(name):
    v, _ = _grid()
    rng = np.random.default_rng(SEEDS[name])
    r = _radius(v)
    if name == "sphere":
        return (r - 0.3).astype(np.float32)[:, None], None
    if name == "noise":
        sign = rng.integers(0, 2, size=v.shape[0]) * 2.0 - 1.0
        mag = rng.uniform(0.25, 1.0, size=v.shape[0])
        sdf = np.where(r < NOISE_RADIUS, sign * mag, mag)
        deformation = 0.3 * rng.normal(size=v.shape)
        return sdf.astype(np.float32)[:, None], deformation.astype(np.float32)
    if name == "zeros":
        sdf = (r - 0.3).astype(np.float32)
        sdf[rng.random(v.shape[0]) < 0.1] = 0.0
        return sdf[:, None], None
    raise KeyError(name)


def case(name):
    sdf, deformation = _case(name)
    return sdf.copy(), None if deformation is None else deformation.copy()


def weights(name, V):
    return np.random.default_rng(SEEDS[name] + 100).normal(size=(int(V), 3)).astype(np.float32)


def case_histogram(sdf, indices):
    """[16] how many tetrahedra take each marching-tetrahedra case (sum over the corners k of (sdf > 0) * 2^k)."""
    occ = (sdf.reshape(-1) > 0)[indices].astype(np.int64)
    return np.bincount((occ * (1 << np.arange(4))).sum(1), minlength=16)


@functools.lru_cache(maxsize=None)
def load_golden():
    """The fixture as a dictionary of arrays (read-only by convention: the tests share it)."""
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
