"""The density field of a Gaussian set, restated densely in float64 numpy from its definition (not from any implementation):

  keep the Gaussians with sigmoid(opacity) > 0.005;  center = (min + max) / 2 of their centres, scale = 1.8 / largest extent (1 for
  a cloud without extent, where the reference divides by zero);
  xyz' = (xyz - center) * scale, std' = exp(scaling) * scale;  Sigma = (R S)(R S)^T with R from the quaternion divided by its norm;
  grid = linspace(-1, 1, R) per axis, in blocks of s = R / num_blocks points;  a Gaussian is a member of a block when xyz' lies
  strictly inside [first - m, last + m] of the block's grid coordinates on all three axes, m = relax_ratio * 2 / num_blocks;
  Sigma^-1 by the adjugate times 1 / (det + 1e-24);  power = -0.5 d^T Sigma^-1 d, weight = exp(power), 0 for a positive power;
  voxel = sum over the members of its block of opacity * weight.

density_field() also reports how close any centre comes to a face of a box it is tested against: a caller that compares a float32
evaluation with this one needs that distance to be far above float32 rounding, or the two may disagree about a member."""
import numpy as np


def _covariance(std, q):
    q = q / np.sqrt((q * q).sum(1, keepdims=True))
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - r * z)
    R[:, 0, 2] = 2 * (x * z + r * y)
    R[:, 1, 0] = 2 * (x * y + r * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - r * x)
    R[:, 2, 0] = 2 * (x * z - r * y)
    R[:, 2, 1] = 2 * (y * z + r * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    L = R * std[:, None, :]
    return L @ L.transpose(0, 2, 1)


def density_field(xyz, opacity_raw, scaling_raw, rotation, resolution, num_blocks, relax_ratio=1.5, voxels=None):
    """(field, info).  field: [R, R, R] float64, or the values at the flat indices `voxels`.  info: center [3], scale, kept (number of
    Gaussians past the prefilter), face_distance (smallest |xyz' - face| over every centre and every box face), members [nb, nb, nb]."""
    R, nb = int(resolution), int(num_blocks)
    assert R % nb == 0
    s = R // nb
    xyz, rotation = np.asarray(xyz, np.float64), np.asarray(rotation, np.float64)
    opacity = 1.0 / (1.0 + np.exp(-np.asarray(opacity_raw, np.float64).reshape(-1)))
    std = np.exp(np.asarray(scaling_raw, np.float64))
    keep = opacity > 0.005
    out = np.zeros(R ** 3) if voxels is None else np.zeros(len(voxels))
    info = dict(center=None, scale=None, kept=int(keep.sum()), face_distance=np.inf, members=np.zeros((nb, nb, nb), np.int64))
    if not keep.any():
        return (out.reshape(R, R, R) if voxels is None else out), info
    xyz, opacity, std, rotation = xyz[keep], opacity[keep], std[keep], rotation[keep]
    mn, mx = xyz.min(0), xyz.max(0)
    extent = (mx - mn).max()
    center, scale = (mn + mx) / 2, (1.8 / extent if extent > 0 else 1.0)      # a cloud without extent is left at its size
    xyz, std = (xyz - center) * scale, std * scale
    cov = _covariance(std, rotation)
    a, b, c, d, e, f = cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]
    inv_det = 1 / (a * d * f + 2 * e * c * b - e ** 2 * a - c ** 2 * d - b ** 2 * f + 1e-24)
    ia, ib, ic = (d * f - e ** 2) * inv_det, (e * c - b * f) * inv_det, (e * b - c * d) * inv_det
    id_, ie, if_ = (a * f - c ** 2) * inv_det, (b * c - e * a) * inv_det, (a * d - b ** 2) * inv_det
    grid = np.linspace(-1, 1, R)
    margin = (2 / nb) * relax_ratio
    lo, hi = grid[0::s] - margin, grid[s - 1::s] + margin            # [nb] each
    inside = (xyz[:, :, None] > lo[None, None, :]) & (xyz[:, :, None] < hi[None, None, :])      # [P, 3, nb]
    info.update(center=center, scale=scale,
                face_distance=float(min(np.abs(xyz[:, :, None] - lo).min(), np.abs(xyz[:, :, None] - hi).min())))
    if voxels is not None:
        voxels = np.asarray(voxels)
        vi, vj, vk = voxels // (R * R), (voxels // R) % R, voxels % R
    for bx in range(nb):
        for by in range(nb):
            for bz in range(nb):
                m = inside[:, 0, bx] & inside[:, 1, by] & inside[:, 2, bz]
                info["members"][bx, by, bz] = int(m.sum())
                if not m.any():
                    continue
                if voxels is None:
                    px, py, pz = (t.reshape(-1) for t in np.meshgrid(grid[bx * s:bx * s + s], grid[by * s:by * s + s],
                                                                     grid[bz * s:bz * s + s], indexing="ij"))
                else:
                    sel = np.nonzero((vi // s == bx) & (vj // s == by) & (vk // s == bz))[0]
                    if sel.size == 0:
                        continue
                    px, py, pz = grid[vi[sel]], grid[vj[sel]], grid[vk[sel]]
                dx, dy, dz = px[:, None] - xyz[m, 0], py[:, None] - xyz[m, 1], pz[:, None] - xyz[m, 2]
                power = -0.5 * (dx ** 2 * ia[m] + dy ** 2 * id_[m] + dz ** 2 * if_[m]) - dx * dy * ib[m] - dx * dz * ic[m] - dy * dz * ie[m]
                val = (opacity[m] * np.where(power > 0, 0.0, np.exp(np.minimum(power, 0.0)))).sum(1)
                if voxels is None:
                    ii, jj, kk = np.meshgrid(np.arange(bx * s, bx * s + s), np.arange(by * s, by * s + s), np.arange(bz * s, bz * s + s),
                                             indexing="ij")
                    out[((ii * R + jj) * R + kk).reshape(-1)] = val
                else:
                    out[sel] = val
    return (out.reshape(R, R, R) if voxels is None else out), info
