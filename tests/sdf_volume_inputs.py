"""Seeded inputs of the NeuS volume-rendering tests (tests/test_sdf_volume_cpu.py, tests/test_gpu_sdf_volume.py).  Small enough for
seconds on the GPU and chosen where the kernels can still go wrong.

composite(): 11 rays with RAY_COUNTS = 0, 1, 63, 64, 65, 0, 128, 129, 200, 353 and 2 samples (M = 1005): a ray count that is no
  multiple of four, empty rays inside, and every side of the 64-lane trip.  Sample lengths in (0, 0.01]; the sdf falls along every ray
  from +0.1 to -0.05, but the samples listed at FORCED (ray, sample) sit at sdf = -0.5, far behind the surface: samples 63, 64 and 128
  of the 129-sample ray (lane 63 of a trip, lane 0 of the next, a trip of one) and every sample from 150 on of the 200-sample ray.
  There alpha is exactly 1 in float32 at beta = 300.  Normals are unit vectors with |d . n| >= MIN_COS, about 30 % of them facing
  away, so that neither relu kink of iter_cos is within reach of a float32 rounding.  values[C] [M, C] and g_out[C] [R, 2 + C] for
  C in CHANNELS (0: no values), g_weights [M].  Variants: BETAS x RHOS x normals present or None x CHANNELS.
pruning(): the samples of volume_inputs' march case c_r257 with the alphas of a sphere of radius 0.3 at beta = 40, computed in
  float64 in the alpha_fn form and rounded once: what the test's alpha_fn hands to OccupancyGrid.sampling.
The arrays are shared between the tests and read-only."""
import functools

import numpy as np

import volume_inputs

RAY_COUNTS = (0, 1, 63, 64, 65, 0, 128, 129, 200, 353, 2)
FORCED = tuple((7, k) for k in (63, 64, 128)) + tuple((8, k) for k in range(150, 200))
BETAS = (20.0, 300.0)
RHOS = (1.0, 0.3)
CHANNELS = (0, 1, 3, 16)
MIN_COS = 0.05
EPS = 1e-5
ALPHA_THRE, EARLY_STOP_EPS = 0.01, 1e-4
PRUNING_BETA, PRUNING_RADIUS = 40.0, 0.3


def _freeze(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def composite():
    """dict: offsets [R + 1], ray_indices [M] int32, n_rays, rays_d [R, 3], t_starts, t_ends, sdf [M], normals [M, 3], g_weights [M]
    float32, and per C in CHANNELS values[C] [M, C] (None for 0) and g_out[C] [R, 2 + C]."""
    rng = np.random.default_rng(3100)
    counts = np.array(RAY_COUNTS)
    R, M = counts.size, int(counts.sum())
    offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int32)
    ray_indices = np.repeat(np.arange(R, dtype=np.int32), counts)
    d = rng.standard_normal((R, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    t_starts, t_ends, sdf = np.zeros(M, np.float32), np.zeros(M, np.float32), np.zeros(M, np.float32)
    for r in range(R):
        a, b = offsets[r], offsets[r + 1]
        delta = rng.uniform(0.001, 0.0099, b - a)
        ts = 1.0 + np.concatenate(([0.0], np.cumsum(delta)[:-1])) if b > a else delta
        t_starts[a:b], t_ends[a:b] = ts, ts + delta
        sdf[a:b] = np.linspace(0.1, -0.05, b - a)
    for r, k in FORCED:
        sdf[offsets[r] + k] = -0.5
    per_sample_d = d[ray_indices].astype(np.float64)
    normals = np.zeros((M, 3))
    todo = np.ones(M, bool)
    while todo.any():                                                # redraw the normals too close to perpendicular
        n = todo.sum()
        facing = np.where(rng.random((n, 1)) < 0.7, 1.0, -1.0)
        draw = -per_sample_d[todo] * facing + 0.4 * rng.standard_normal((n, 3))
        normals[todo] = draw / np.linalg.norm(draw, axis=1, keepdims=True)
        todo = np.abs((per_sample_d * normals.astype(np.float32)).sum(1)) < 1.2 * MIN_COS
    case = dict(offsets=offsets, ray_indices=ray_indices, n_rays=R, rays_d=d, t_starts=t_starts, t_ends=t_ends, sdf=sdf,
                normals=normals.astype(np.float32), g_weights=rng.standard_normal(M, dtype=np.float32),
                values={C: rng.standard_normal((M, C), dtype=np.float32) if C else None for C in CHANNELS},
                g_out={C: rng.standard_normal((R, 2 + C), dtype=np.float32) for C in CHANNELS})
    for group in (case, case["values"], case["g_out"]):
        _freeze(group)
    return case


def variants():
    """(beta, rho, with_normals, C) of every variant of the compositing case."""
    return [(beta, rho, n, C) for beta in BETAS for rho in RHOS for n in (True, False) for C in CHANNELS]


@functools.lru_cache(maxsize=None)
def pruning():
    """dict: the samples of c_r257 (ray_indices, t_starts, t_ends, offsets, n_rays) and alphas [M] float32."""
    case = volume_inputs.march_case("c_r257")
    ray_indices, t_starts, t_ends, offsets = volume_inputs.marched("c_r257")
    ts, te = t_starts.astype(np.float64), t_ends.astype(np.float64)
    p = case["rays_o"][ray_indices].astype(np.float64) + case["rays_d"][ray_indices] * ((ts + te) / 2)[:, None]
    sdf = np.sqrt((p * p).sum(1)) - PRUNING_RADIUS
    step = te - ts
    c = 1 / (1 + np.exp(-(sdf + step * 0.5) * PRUNING_BETA))
    m = 1 / (1 + np.exp(-(sdf - step * 0.5) * PRUNING_BETA))
    alphas = np.clip((c - m + EPS) / (c + EPS), 0.0, 1.0).astype(np.float32)
    return _freeze(dict(ray_indices=ray_indices, t_starts=t_starts, t_ends=t_ends, offsets=offsets, n_rays=257, alphas=alphas))
