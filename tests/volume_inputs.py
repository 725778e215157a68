"""Seeded inputs of the volume-rendering tests (tests/test_volume_cpu.py, tests/test_gpu_volume.py).  Every case is small enough for
seconds on the GPU and chosen where the kernels can still go wrong.

March cases; a case is a dict(rays_o, rays_d [R, 3], occ [G, G, G] uint8, lo, hi [3], dt, near, far, jitter [R] or None, K_cap):
  a            R 65, G 8, a random half-full grid over an off-centre box, origins outside it, no jitter; 150 to 330 candidates a ray.
  b            the same with jitter.
  c_r1, c_r63, c_r257   G 32 over [-1, 1]^3 with a sphere of radius 0.6 occupied, 1, 63 and 257 rays aimed near the centre.
  d_edge       the edge rays listed at EDGE_RAYS through a random half-full 4^3 grid;
  d_zeros, d_ones, d_kcap, d_far   the same rays through an all-zero and an all-ones grid, with K_cap 10 (below every hit ray's
               candidates) and with far = 2.5, which cuts t_far inside the box.
  trips        an all-ones grid and rays along +x from inside the box that have exactly TRIP_COUNTS = 0, 1, 63, 64, 65, 129 and 200
               samples (origin x = 1 - n / 128 with dt = 1 / 128, all exact in float32), then 9 random rays: every side of the 64-lane trip.
  e_r0         no ray.
Compositing: composite() gives, on the samples of `trips` (marched by the restatement), sigmas in [0, 50], values with C = 1, 3, 4
and 16 and upstream gradients for the weights and for every accumulated output.  pruning() gives the samples of c_r257 with a smooth
density for OccupancyGrid.sampling.  The arrays are shared between the tests and read-only."""
import functools

import numpy as np

MARCH_CASES = ("a", "b", "c_r1", "c_r63", "c_r257", "d_edge", "d_zeros", "d_ones", "d_kcap", "d_far", "trips", "e_r0")
TRIP_COUNTS = (0, 1, 63, 64, 65, 129, 200)
CHANNELS = (1, 3, 4, 16)
ALPHA_THRE, EARLY_STOP_EPS = 0.01, 1e-4
NAN, INF = float("nan"), float("inf")

# (origin, direction, what it is) of case d, over the box [-1, 1]^3
EDGE_RAYS = (
    ((0.1, 0.2, -0.3), (0.3, -0.5, 0.8), "origin inside the box"),
    ((-3.0, 0.2, 0.1), (1.0, 0.0, 0.1), "one zero component, inside its slab"),
    ((-3.0, 1.5, 0.1), (1.0, 0.0, 0.1), "one zero component, outside its slab"),
    ((-3.0, 0.2, 0.1), (1.0, 0.0, 0.0), "two zero components, inside their slabs"),
    ((-3.0, 0.2, 1.5), (1.0, 0.0, 0.0), "two zero components, outside one slab"),
    ((-3.0, -1.0, 1.0), (1.0, 0.0, -0.0), "zero components (one a negative zero) with the origin exactly on lo and on hi"),
    ((-1.0, 0.3, 0.2), (1.0, 0.1, 0.2), "origin exactly on a face, pointing in"),
    ((1.0, 0.0, 0.0), (1.0, 0.0, 0.0), "origin exactly on a face, pointing out"),
    ((-3.0, 3.0, 0.0), (1.0, 0.1, 0.0), "a miss"),
    ((-3.0, 0.0, 0.0), (-1.0, 0.1, 0.0), "the box lies behind the origin"),
    ((3.0, 2.5, -2.0), (-0.9, -0.7, 0.6), "a diagonal ray with negative components"),
    ((-3.0, 0.2, 0.1), (2.0, 0.0, 0.0), "a direction that is not unit"),
    ((-3.0, 0.2, 0.1), (1.0, 1e-45, 0.0), "a denormal component: 1 / d is infinite"),
    ((-3.0, -1.0, 0.1), (1.0, 1e-45, 0.0), "a denormal component with lo - o == 0: 0 x inf is a NaN"),
    ((NAN, 0.0, 0.0), (1.0, 0.0, 0.0), "NaN origin"),
    ((-3.0, INF, 0.0), (1.0, 0.0, 0.0), "infinite origin"),
    ((-3.0, 0.0, 0.0), (1.0, NAN, 0.0), "NaN direction"),
    ((-3.0, 0.0, 0.0), (-INF, 0.0, 0.0), "infinite direction"),
    ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), "zero direction, inside the box"),
    ((-3.0, 0.1, 0.2), (0.0, -0.0, 0.0), "zero direction, outside the box"),
)


def _freeze(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def _aimed_rays(rng, R, distance, spread):
    """R origins on the sphere of radius `distance`, each looking at a point within `spread` of the centre; unit directions."""
    o = rng.standard_normal((R, 3))
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * distance
    d = rng.uniform(-spread, spread, (R, 3)) - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


def _sphere_grid(G, radius):
    c = (np.arange(G) + 0.5) / G * 2 - 1
    x, y, z = np.meshgrid(c, c, c, indexing="ij")
    return (x * x + y * y + z * z <= radius * radius).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def march_case(name):
    assert name in MARCH_CASES, name
    rng = np.random.default_rng(2000 + MARCH_CASES.index(name))
    unit_lo, unit_hi = np.full(3, -1, np.float32), np.full(3, 1, np.float32)
    if name in ("a", "b"):
        rng = np.random.default_rng(2000)                            # b is a with jitter
        o, d = _aimed_rays(rng, 65, 3.5, 0.5)
        case = dict(rays_o=o, rays_d=d, occ=(rng.random((8, 8, 8)) < 0.5).astype(np.uint8), lo=np.array([-1, -0.8, -1.2], np.float32),
                    hi=np.array([1, 1.1, 0.9], np.float32), dt=0.01, near=0.0, far=1e10, jitter=None, K_cap=1024)
        if name == "b":
            case["jitter"] = np.random.default_rng(2001).random(65, dtype=np.float32)
    elif name.startswith("c_r"):
        o, d = _aimed_rays(rng, int(name[3:]), 3.0, 0.7)
        case = dict(rays_o=o, rays_d=d, occ=_sphere_grid(32, 0.6), lo=unit_lo, hi=unit_hi, dt=1.732 * 2 / 256, near=0.0, far=1e10, jitter=None,
                    K_cap=1024)
    elif name.startswith("d_"):
        o = np.array([r[0] for r in EDGE_RAYS], np.float32)
        d = np.array([r[1] for r in EDGE_RAYS], np.float32)
        occ = (np.random.default_rng(2005).random((4, 4, 4)) < 0.5).astype(np.uint8)
        if name == "d_zeros":
            occ = np.zeros_like(occ)
        elif name != "d_edge":
            occ = np.ones_like(occ)
        case = dict(rays_o=o, rays_d=d, occ=occ, lo=unit_lo, hi=unit_hi, dt=0.03, near=0.0, far=2.5 if name == "d_far" else 1e10, jitter=None,
                    K_cap=10 if name == "d_kcap" else 1024)
    elif name == "trips":
        n = np.array(TRIP_COUNTS, np.float32)
        o = np.stack((1 - n / 128, rng.uniform(-0.9, 0.9, n.size).astype(np.float32), rng.uniform(-0.9, 0.9, n.size).astype(np.float32)), axis=1)
        d = np.tile(np.array([[1, 0, 0]], np.float32), (n.size, 1))
        o2, d2 = _aimed_rays(rng, 9, 2.5, 0.8)
        case = dict(rays_o=np.concatenate((o, o2)).astype(np.float32), rays_d=np.concatenate((d, d2)), occ=np.ones((8, 8, 8), np.uint8),
                    lo=unit_lo, hi=unit_hi, dt=1.0 / 128, near=0.0, far=1e10, jitter=None, K_cap=1024)
    else:
        case = dict(rays_o=np.zeros((0, 3), np.float32), rays_d=np.zeros((0, 3), np.float32), occ=np.ones((8, 8, 8), np.uint8), lo=unit_lo,
                    hi=unit_hi, dt=0.01, near=0.0, far=1e10, jitter=None, K_cap=1024)
    case["scale"] = (np.float32(case["occ"].shape[0]) / (case["hi"] - case["lo"])).astype(np.float32)        # as march_rays computes it
    return _freeze(case)


@functools.lru_cache(maxsize=None)
def marched(name):
    """(ray_indices, t_starts, t_ends, offsets) of a march case by the restatement.  Computed once and shared."""
    import volume_reference as reference
    out = reference.march(march_case(name))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def composite():
    """dict: the samples of `trips` (ray_indices, t_starts, t_ends, offsets, n_rays), sigmas [M] in [0, 50], g_weights [M], and per
    C in CHANNELS values[C] [M, C] and g_out[C] [n_rays, C]."""
    ray_indices, t_starts, t_ends, offsets = marched("trips")
    rng = np.random.default_rng(2100)
    M, R = ray_indices.shape[0], offsets.shape[0] - 1
    case = dict(ray_indices=ray_indices, t_starts=t_starts, t_ends=t_ends, offsets=offsets, n_rays=R,
                sigmas=(rng.random(M, dtype=np.float32) * 50).astype(np.float32), g_weights=rng.standard_normal(M, dtype=np.float32),
                values={C: rng.standard_normal((M, C), dtype=np.float32) for C in CHANNELS},
                g_out={C: rng.standard_normal((R, C), dtype=np.float32) for C in CHANNELS})
    for group in (case, case["values"], case["g_out"]):
        _freeze(group)
    return case


@functools.lru_cache(maxsize=None)
def pruning():
    """dict: the samples of c_r257 and sigmas [M] = 80 exp(-|p|^2 / (2 x 0.15^2)) at their midpoints p, float32 (computed in float64
    and rounded once): what the test's sigma_fn hands to OccupancyGrid.sampling."""
    case = march_case("c_r257")
    ray_indices, t_starts, t_ends, offsets = marched("c_r257")
    tm = (t_starts.astype(np.float64) + t_ends) / 2
    p = case["rays_o"][ray_indices].astype(np.float64) + case["rays_d"][ray_indices] * tm[:, None]
    sigmas = (80.0 * np.exp(-(p * p).sum(1) / (2 * 0.15 ** 2))).astype(np.float32)
    return _freeze(dict(ray_indices=ray_indices, t_starts=t_starts, t_ends=t_ends, offsets=offsets, n_rays=257, sigmas=sigmas))
