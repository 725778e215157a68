"""Seeded scenes of the mesh rasterizer tests (tests/test_mesh_render_cpu.py, tests/test_gpu_mesh_render.py): clip-space positions
[V, 4] float32 and triangles [F, 3] int32.  A vertex is placed at an NDC point with its own w (1 .. 20: a strongly perspective view)
and depth z/w, and stored as (ndc_x w, ndc_y w, zw w, w)."""
import numpy as np

H, W = 45, 67             # neither a multiple of 8 or 64, and W != H
GRID = (9, 7)             # vertices per row, rows


def _clip(ndc_xy, zw, w):
    ndc_xy, zw, w = np.asarray(ndc_xy, np.float64), np.asarray(zw, np.float64), np.asarray(w, np.float64)
    return np.concatenate((ndc_xy * w[:, None], (zw * w)[:, None], w[:, None]), 1).astype(np.float32)


def grid_mesh(seed, on_centres=False, h=H, w=W):
    """(pos [63, 4], tri [96, 3]): a triangulated 9 x 7 vertex grid that covers the image, its border vertices outside it.  Interior
    vertices are jittered by up to 0.3 cell; on_centres: every vertex exactly on a pixel centre instead (w = 1).  Half of the triangles
    have their winding flipped, and each cell is split along a random diagonal."""
    rng = np.random.default_rng(seed)
    nx, ny = GRID
    if on_centres:
        px = np.round(np.linspace(-1, w, nx))
        py = np.round(np.linspace(-1, h, ny))
        gx, gy = np.meshgrid((2 * px + 1) / w - 1, (2 * py + 1) / h - 1)
        ww = np.ones(nx * ny)
    else:
        gx, gy = np.meshgrid(np.linspace(-1.15, 1.15, nx), np.linspace(-1.15, 1.15, ny))
        jx, jy = rng.uniform(-0.3, 0.3, (2, ny, nx)) * np.array([2.3 / (nx - 1), 2.3 / (ny - 1)])[:, None, None]
        jx[[0, -1], :] = jy[[0, -1], :] = jx[:, [0, -1]] = jy[:, [0, -1]] = 0
        gx, gy = gx + jx, gy + jy
        ww = rng.uniform(1, 20, nx * ny)
    pos = _clip(np.stack((gx.ravel(), gy.ravel()), 1), rng.uniform(0.3, 0.9, nx * ny), ww)
    tri = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a, b, c, d = j * nx + i, j * nx + i + 1, (j + 1) * nx + i, (j + 1) * nx + i + 1
            pair = [(a, b, d), (a, d, c)] if rng.random() < 0.5 else [(a, b, c), (b, d, c)]
            tri += [t if rng.random() < 0.5 else t[::-1] for t in pair]
    return pos, np.array(tri, np.int32)


class _Builder:
    def __init__(self, pos, tri):
        self.pos, self.tri, self.tags = [pos], [tri], {}
        self.V, self.F = len(pos), len(tri)

    def add(self, tag, ndc_xy, zw, w):
        """Triangles over their own vertices: ndc_xy [K, 3, 2], zw and w [K, 3]."""
        k = len(ndc_xy)
        self.pos.append(_clip(np.reshape(ndc_xy, (-1, 2)), np.reshape(zw, -1), np.reshape(w, -1)))
        self.tri.append((self.V + np.arange(3 * k)).reshape(k, 3).astype(np.int32))
        self.tags[tag] = np.arange(self.F, self.F + k)
        self.V += 3 * k
        self.F += k


def coverage_scene(seed):
    """(pos [V, 4], tri [F, 3], tags: name -> triangle ids) of one view: the jittered grid, 200 random triangles (some partly, some
    wholly off-screen), sub-pixel triangles around pixel corners, a zero-area triangle, triangles with a vertex at w <= 0, one beyond
    the guard band, triangles at depths outside [-1, 1] (wholly and partly), two coincident triangles at one depth, and two
    interpenetrating triangles that each fill the screen.  The topology does not depend on the seed."""
    rng = np.random.default_rng(seed)
    b = _Builder(*grid_mesh(1000 + seed))
    b.tri[0] = grid_mesh(1000)[1]                                   # one topology for every view
    c = rng.uniform(-1.4, 1.4, (200, 1, 2))
    b.add("random", c + rng.uniform(-1, 1, (200, 3, 2)) * rng.uniform(0.02, 0.8, (200, 1, 1)), rng.uniform(-0.9, 0.9, (200, 3)),
          rng.uniform(1, 20, (200, 3)))
    corner = np.stack((2 * rng.integers(1, W - 1, 20) / W - 1, 2 * rng.integers(1, H - 1, 20) / H - 1), 1)[:, None, :]
    b.add("subpixel", corner + rng.uniform(-0.2, 0.2, (20, 3, 2)) * np.array([2 / W, 2 / H]), np.full((20, 3), -0.95), rng.uniform(1, 20, (20, 3)))
    big = np.array([[-0.8, -0.7], [0.9, -0.5], [0.1, 0.8]])
    b.add("zero_area", [[big[0], big[1], big[1]]], np.full((1, 3), -0.99), [[2.0, 3.0, 3.0]])
    b.add("behind", [big, big], np.full((2, 3), -0.99), [[1.0, -1.0, 2.0], [1.0, 2.0, 0.0]])
    b.add("guard_band", [[big[0], [2000.0, 0.3], big[2]]], np.full((1, 3), -0.99), [[1.0, 2.0, 3.0]])
    b.add("depth_out", [big, big, big], [[1.5, 1.5, 1.5], [-0.6, 1.5, -0.3], [-1.5, -0.2, -0.4]], rng.uniform(1, 20, (3, 3)))
    same = big * 0.6 + rng.uniform(-0.2, 0.2, 2)
    b.add("coincident", [same, same], np.full((2, 3), -0.5), np.tile(rng.uniform(1, 20, 3), (2, 1)))
    b.add("screen_filling", [[[-3.5, -3.0], [3.5, -3.0], [0.0, 3.5]], [[3.5, 3.0], [-3.5, 3.0], [0.0, -3.5]]],
          [[0.3, 0.95, 0.6], [0.3, 0.95, 0.65]], [[1.0, 1.0, 1.0], [1.0, 2.0, 1.5]])
    return np.concatenate(b.pos), np.concatenate(b.tri), b.tags


def coverage_views(B=2):
    """(pos [B, V, 4], tri [F, 3], tags)."""
    views = [coverage_scene(s) for s in range(B)]
    assert all(np.array_equal(v[1], views[0][1]) for v in views)
    return np.stack([v[0] for v in views]), views[0][1], views[0][2]


def grid_views(B=2):
    """(pos [B, 63, 4], tri [96, 3]) of the jittered grid alone."""
    tri = grid_mesh(1000)[1]
    return np.stack([grid_mesh(1000 + s)[0] for s in range(B)]), tri


# render_mesh reads a camera's full_proj_transform (row-vector convention).  With this one, a world vertex (x, y, z) becomes the clip
# position (x, y, 0.5, z) EXACTLY (every product is by 0 or 1), so a test knows the positions render_mesh rasterizes bit for bit.
EXACT_PROJ = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 0.5, 0]], np.float32)


def world_of(pos):
    """World vertices [V, 3] whose clip positions under EXACT_PROJ are (x, y, 0.5, w) of pos [V, 4] (needs w >= 0.5 for a depth <= 1)."""
    return np.ascontiguousarray(pos[:, [0, 1, 3]])


def exact_clip(world):
    out = np.empty((len(world), 4), np.float32)
    out[:, :2], out[:, 2], out[:, 3] = world[:, :2], 0.5, world[:, 2]
    return out
