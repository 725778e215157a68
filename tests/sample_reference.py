"""The three sums of csrc/field_sample.hip at arbitrary points, restated densely in numpy from their definition (not from any
implementation), in float64 or — the same statements in the other precision — float32:

  sources, normalisation, covariance and its adjugate inverse A: those of tests/field_reference.py (the density field's);
  a query point x (normalised coordinates) is evaluated in a block b that the caller names;  a Gaussian is a member of b when its
  normalised centre lies strictly inside [first - m, last + m] of the block's grid coordinates on all three axes — tested in
  float32 on float32 values (grid = torch.linspace(-1, 1, R), m = relax_ratio * 2 / num_blocks), as the reference tests it;
  d = x - mu', power = -0.5 d^T A d, w = opacity * exp(power), 0 for a positive power;  over the members of b:
      density = sum w        gradient = sum w * (-A d)        color_sum = sum w * rgb

Dense over the Gaussians: every point meets every Gaussian and non-members are masked.  `face_distance` (float64) is how close any
centre comes to a box face: far above float32 rounding, both precisions agree about every member and differ by rounding alone."""
import numpy as np
import torch


def _covariance(std, q):
    """Sigma = (R S)(R S)^T with R from the quaternion divided by its norm, in the dtype of the inputs."""
    q = q / np.sqrt((q * q).sum(1, keepdims=True))
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = q.dtype.type(1), q.dtype.type(2)
    R = np.empty((q.shape[0], 3, 3), q.dtype)
    R[:, 0, 0] = one - two * (y * y + z * z)
    R[:, 0, 1] = two * (x * y - r * z)
    R[:, 0, 2] = two * (x * z + r * y)
    R[:, 1, 0] = two * (x * y + r * z)
    R[:, 1, 1] = one - two * (x * x + z * z)
    R[:, 1, 2] = two * (y * z - r * x)
    R[:, 2, 0] = two * (x * z - r * y)
    R[:, 2, 1] = two * (y * z + r * x)
    R[:, 2, 2] = one - two * (x * x + y * y)
    L = R * std[:, None, :]
    return L @ L.transpose(0, 2, 1)


def point_blocks(u, resolution, num_blocks):
    """Block id ((bx * nb + by) * nb + bz, int64) of normalised float32 points by the rule of GaussianModel.sample_fields: per axis
    the last grid value <= the coordinate, clamped to the grid, in blocks of resolution / num_blocks."""
    grid = torch.linspace(-1, 1, resolution, dtype=torch.float32)
    cell = (torch.bucketize(torch.from_numpy(np.ascontiguousarray(u, np.float32)), grid, right=True) - 1).clamp(0, resolution - 1)
    cell = (cell // (resolution // num_blocks)).numpy().astype(np.int64)
    return (cell[:, 0] * num_blocks + cell[:, 1]) * num_blocks + cell[:, 2]


def sample_sums(xyz, opacity_raw, scaling_raw, rotation, rgb, resolution, num_blocks, points, blocks, relax_ratio=1.5, dtype=np.float64,
                chunk=512):
    """(density [V], gradient [V, 3], color_sum [V, 3], info) in `dtype` at the normalised `points` [V, 3], point i evaluated in block
    blocks[i].  rgb: [P, 3] per Gaussian (before the prefilter).  info: center, scale, kept, face_distance, members [nb^3]."""
    R, nb, T = int(resolution), int(num_blocks), dtype
    s = R // nb
    xyz, rotation = np.asarray(xyz, T), np.asarray(rotation, T)
    opacity = (1 / (1 + np.exp(-np.asarray(opacity_raw, T).reshape(-1)))).astype(T)
    std = np.exp(np.asarray(scaling_raw, T))
    keep = opacity > T(0.005)
    points, blocks = np.asarray(points, T), np.asarray(blocks, np.int64)
    V = points.shape[0]
    dens, grad, csum = np.zeros(V, T), np.zeros((V, 3), T), np.zeros((V, 3), T)
    info = dict(center=None, scale=None, kept=int(keep.sum()), keep=keep, face_distance=np.inf, members=np.zeros(nb ** 3, np.int64))
    if not keep.any():
        return dens, grad, csum, info
    xyz, opacity, std, rotation, rgb = xyz[keep], opacity[keep], std[keep], rotation[keep], np.asarray(rgb, T)[keep]
    mn, mx = xyz.min(0), xyz.max(0)
    extent = (mx - mn).max()
    center, scale = (mn + mx) / T(2), (T(1.8) / extent if extent > 0 else T(1.0))
    xyz, std = ((xyz - center) * scale).astype(T), (std * scale).astype(T)
    cov = _covariance(std, rotation)
    assert cov.dtype == T
    a, b, c, d, e, f = cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]
    inv_det = T(1) / (a * d * f + T(2) * e * c * b - e ** 2 * a - c ** 2 * d - b ** 2 * f + T(1e-24))
    ia, ib, ic = (d * f - e ** 2) * inv_det, (e * c - b * f) * inv_det, (e * b - c * d) * inv_det
    id_, ie, if_ = (a * f - c ** 2) * inv_det, (b * c - e * a) * inv_det, (a * d - b ** 2) * inv_det
    # membership: float32 values, float32 comparisons
    grid = torch.linspace(-1, 1, R, dtype=torch.float32).numpy()
    margin = np.float32((2 / nb) * relax_ratio)
    lo, hi = grid[0::s] - margin, grid[s - 1::s] + margin                        # [nb] float32
    x32 = xyz.astype(np.float32)
    inside = (x32[:, :, None] > lo[None, None, :]) & (x32[:, :, None] < hi[None, None, :])      # [P, 3, nb]
    if T is np.float64:
        lo64 = np.linspace(-1, 1, R)[0::s] - (2 / nb) * relax_ratio
        hi64 = np.linspace(-1, 1, R)[s - 1::s] + (2 / nb) * relax_ratio
        info["face_distance"] = float(min(np.abs(xyz[:, :, None] - lo64).min(), np.abs(xyz[:, :, None] - hi64).min()))
    ids = np.arange(nb ** 3)
    member = inside[:, 0, ids // (nb * nb)] & inside[:, 1, (ids // nb) % nb] & inside[:, 2, ids % nb]      # [P, nb^3]
    info.update(center=center, scale=scale, members=member.sum(0))
    for st in range(0, V, chunk):
        sl = slice(st, min(st + chunk, V))
        m = member[:, blocks[sl]].T                                               # [v, P]
        dx, dy, dz = (points[sl, k:k + 1] - xyz[None, :, k] for k in range(3))
        power = T(-0.5) * (dx ** 2 * ia + dy ** 2 * id_ + dz ** 2 * if_) - dx * dy * ib - dx * dz * ic - dy * dz * ie
        w = np.where(m & ~(power > 0), opacity * np.exp(np.minimum(power, T(0))), T(0)).astype(T)
        dens[sl] = w.sum(1)
        grad[sl, 0] = (w * -(ia * dx + ib * dy + ic * dz)).sum(1)
        grad[sl, 1] = (w * -(ib * dx + id_ * dy + ie * dz)).sum(1)
        grad[sl, 2] = (w * -(ic * dx + ie * dy + if_ * dz)).sum(1)
        csum[sl] = w @ rgb
    return dens, grad, csum, info
