"""Small scenes whose image is no multiple of the 16 x 16 tile: the last tile column and / or row is only partly inside
the image, its lists are several 64-entry segments long and its inside pixels walk at least two segments deep.

  "cut_both"      41 x 27: both axes cut inside an 8 x 8 quadrant (W % 16 = 11, H % 16 = 9), H * W = 1107 is odd (the planes
                  of a second view start 4-byte aligned), four of the six tiles are partial.
  "one_pixel"     17 x 33: one pixel row and one pixel column in the last tiles, a 1 x 1 corner tile.
  "sub_quadrant"  9 x 5: the image is smaller than a quadrant; one tile; W < 8.
  "half_tile"     24 x 40: multiples of 8 and not of 16; whole quadrants lie outside, none is cut.
  "wide"          50 x 75: many full tiles next to the partial ones; the rows of the Gaussians that live in the partial tiles
                  alone are far below the tensor maximum.
  "empty_edges"   41 x 27: every Gaussian (3-sigma rectangle included) inside tile (0, 0); every partial tile's list is empty.

The ball population is scenes.make_scene("ball", P, seed=5, sh_degree=1) with random rotations, scales times
s * exp(U(-0.7, 0.7)) and opacities U(lo, hi).  "one_pixel" and "wide" get a second population of small splats whose
centres lie in the partial strip, also beyond the last pixel row / column (inside the rounded-up tile), so that many
Gaussians have every tile instance in a partial tile (edge_rows) and some reach the image with their tail alone.
In "one_pixel" such a Gaussian is at least its radius r = ceil(3 sigma_max) away from the single pixel row / column it can
reach (its rectangle would otherwise touch the full tile before it), so G <= exp(-4.5) there: it passes the
alpha >= 1/255 test only with an opacity above (1/255) / exp(-4.5) = 0.353, with 3 sigma_max just below the integer r and
the centre just beyond r.  The rasterizer also floors the discriminant of the eigenvalues at 0.1, which widens the radius
of every nearly round splat.  Random sizes almost never meet all that, so this population is made to: a flat disc facing
the camera with its axes along the image axes, 3 sigma = r - 0.02 (r = 3 or 4, the 0.3 blur included) towards the image and
sigma^2 = 0.31 along the edge, the centre r + U(0.005, 0.12) pixels from the pixel line, opacity U(0.7, 0.95): alpha is
0.0045-0.010 at the nearest pixel.  One such population is made for each camera the GPU tests use.

tests/test_edge_tile_scenes_cpu.py asserts these properties with the CPU oracle alone; tests/test_gpu_edge_tiles.py compares
the HIP forward and backward with the oracle on them."""
import functools

import numpy as np

import scenes

BG = (0.3, 0.1, 0.2)
SH_DEGREE = 1
SEED = 5
#                   P (of the ball population), H, W, scale, opacity range, camera (elevation, distance, fovy)
SCENES = {
    "cut_both":     (1500, 41, 27, 0.6, 0.05, 0.4, (0.0, 1.2, 40.0)),
    "one_pixel":    (1500, 17, 33, 0.6, 0.05, 0.4, (0.0, 0.7, 60.0)),
    "sub_quadrant": (600, 9, 5, 0.5, 0.05, 0.3, (0.0, 1.2, 40.0)),
    "half_tile":    (1500, 24, 40, 0.7, 0.05, 0.4, (0.0, 0.8, 45.0)),
    "wide":         (3000, 50, 75, 0.6, 0.05, 0.4, (0.0, 0.8, 50.0)),
    "empty_edges":  (200, 41, 27, None, 0.05, 0.3, (0.0, 1.2, 40.0)),
}
# the second population, per camera: splats, then either (sigma range in pixels, opacity range, how far the centres lie behind
# the first pixel row / column of the partial tile at least and how far beyond the image's last pixel row / column at most)
# or "tail": the construction of the module docstring
STRIP = {
    "one_pixel": (300, "tail"),
    "wide": (250, 0.6, 1.2, 0.05, 0.3, 3.0, 2.5),
}
N_CULLED = 8                # "empty_edges": Gaussians whose rectangle lies left of the image (radii 0, no instance)
# the cameras the GPU tests use: azimuth 0 everywhere, a second view for the two-view launch sets
SECOND_AZIMUTH = {"cut_both": 90.0, "one_pixel": 120.0}


def azimuths(name):
    return (0.0, SECOND_AZIMUTH[name]) if name in SECOND_AZIMUTH else (0.0,)


def camera(name, azimuth=0.0):
    P, H, W = SCENES[name][:3]
    el, dist, fovy = SCENES[name][6]
    return scenes.camera(el, azimuth, dist, fovy, H, W)


def _camera_quaternion(cam):
    """(r, x, y, z) of the rotation whose columns are the camera's axes in space (a mirrored axis turned back: a Gaussian's
    covariance does not see the sign of an axis)."""
    R = cam["viewmatrix"].astype(np.float64)[:3, :3].copy()
    if np.linalg.det(R) < 0:
        R[:, 2] = -R[:, 2]
    K = np.array([[R[0, 0] - R[1, 1] - R[2, 2], R[1, 0] + R[0, 1], R[2, 0] + R[0, 2], R[2, 1] - R[1, 2]],
                  [R[1, 0] + R[0, 1], R[1, 1] - R[0, 0] - R[2, 2], R[2, 1] + R[1, 2], R[0, 2] - R[2, 0]],
                  [R[2, 0] + R[0, 2], R[2, 1] + R[1, 2], R[2, 2] - R[0, 0] - R[1, 1], R[1, 0] - R[0, 1]],
                  [R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], R[0, 0] + R[1, 1] + R[2, 2]]]) / 3.0
    x, y, z, r = np.linalg.eigh(K)[1][:, -1]
    return np.array([r, x, y, z])


def _tail_discs(sc, cam, H, W, z, r, n_col):
    """Turns the Gaussians of `sc` into the discs of the module docstring: the first n_col reach towards -x, the rest
    towards -y."""
    n = z.shape[0]
    fx, fy = W / (2.0 * cam["tanfovx"]), H / (2.0 * cam["tanfovy"])
    towards = np.sqrt(((r - 0.02) / 3.0) ** 2 - 0.3)
    along = np.full(n, np.sqrt(0.31 - 0.3))
    col = np.arange(n) < n_col
    sx, sy = np.where(col, towards, along) * z / fx, np.where(col, along, towards) * z / fy
    sc["scales"] = np.stack([sx, sy, 1e-3 * np.minimum(sx, sy)], 1).astype(np.float32)
    sc["rotations"] = np.tile(_camera_quaternion(cam), (n, 1)).astype(np.float32)


def _strip(name, rng, azimuth):
    """The second population: centres in the partial strip of the given camera, two thirds of them in the last tile
    column, all depths distinct and inside the ball's depth range."""
    P, H, W = SCENES[name][:3]
    n = STRIP[name][0]
    cam = camera(name, azimuth)
    dist = SCENES[name][6][1]
    x0, y0 = (W // 16) * 16, (H // 16) * 16
    n_col = (2 * n) // 3
    z = dist - 0.3 + 0.6 * (rng.permutation(n) + 0.5) / n
    if STRIP[name][1] == "tail":
        r = rng.integers(3, 5, n).astype(np.float64)
        d = r + rng.uniform(0.005, 0.12, n)
        px = np.r_[W - 1 + d[:n_col], rng.integers(0, W, n - n_col) + rng.uniform(-0.2, 0.2, n - n_col)]
        py = np.r_[rng.integers(0, H, n_col) + rng.uniform(-0.2, 0.2, n_col), H - 1 + d[n_col:]]
        sc = scenes.gaussians_at_pixels(rng, cam, H, W, px, py, z, np.ones(n), rng.uniform(0.7, 0.95, n), SH_DEGREE)
        _tail_discs(sc, cam, H, W, z, r, n_col)
        return sc
    sig_lo, sig_hi, lo, hi, d0, beyond = STRIP[name][1:]
    px = np.r_[x0 + rng.uniform(d0, W - 1 - x0 + beyond, n_col), rng.uniform(0.0, W + 1.0, n - n_col)]
    py = np.r_[rng.uniform(0.0, H + 1.0, n_col), y0 + rng.uniform(d0, H - 1 - y0 + beyond, n - n_col)]
    return scenes.gaussians_at_pixels(rng, cam, H, W, px, py, z, rng.uniform(sig_lo, sig_hi, n), rng.uniform(lo, hi, n), SH_DEGREE)


def _inside_tile_0(rng):
    """"empty_edges": centres 4.5-11.5 pixels inside tile (0, 0) and at most 1.2 pixels wide (3-sigma radius <= 4), then
    N_CULLED more whose rectangle lies left of the image."""
    P, H, W = SCENES["empty_edges"][:3]
    lo, hi = SCENES["empty_edges"][4:6]
    cam = camera("empty_edges")
    n = P - N_CULLED
    px = np.r_[rng.uniform(4.5, 11.5, n), rng.uniform(-30.0, -20.0, N_CULLED)]
    py = np.r_[rng.uniform(4.5, 11.5, n), rng.uniform(4.5, 11.5, N_CULLED)]
    z = 1.2 + 0.002 * rng.permutation(P)
    return scenes.gaussians_at_pixels(rng, cam, H, W, px, py, z, rng.uniform(0.6, 1.2, P), rng.uniform(lo, hi, P), SH_DEGREE)


@functools.lru_cache(maxsize=None)
def _build(name):
    P, H, W, s, lo, hi = SCENES[name][:6]
    rng = np.random.default_rng(SEED)
    if name == "empty_edges":
        return _inside_tile_0(rng)
    sc = scenes.make_scene("ball", P, seed=SEED, sh_degree=SH_DEGREE)
    sc["scales"] = (sc["scales"] * s * np.exp(rng.uniform(-0.7, 0.7, (P, 3)))).astype(np.float32)
    q = rng.normal(size=(P, 4))
    sc["rotations"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    sc["opacities"] = rng.uniform(lo, hi, (P, 1)).astype(np.float32)
    if name in STRIP:
        extra = [_strip(name, rng, az) for az in azimuths(name)]
        sc = {k: np.ascontiguousarray(np.concatenate([sc[k]] + [e[k] for e in extra])) for k in sc}
    return sc


def build(name, azimuth=0.0):
    """(scene dict of float32 arrays, camera, H, W) of the named scene; `azimuth` turns the camera.  The arrays are built
    once and shared by every test that asks for the scene: callers do not write to them."""
    P, H, W = SCENES[name][:3]
    return dict(_build(name)), camera(name, azimuth), H, W


def oracle_forward(oracle, name, azimuth=0.0):
    """The oracle's forward of the scene: (RasterOracle with its state, (color, radii, depth, alpha))."""
    sc, cam, H, W = build(name, azimuth)
    ro = oracle.RasterOracle()
    out = ro.forward(image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=np.asarray(BG, np.float32),
                     scale_modifier=1.0, viewmatrix=cam["viewmatrix"], projmatrix=cam["projmatrix"], sh_degree=SH_DEGREE,
                     campos=cam["campos"], means3D=sc["means3D"], opacities=sc["opacities"], shs=sc["shs"],
                     scales=sc["scales"], rotations=sc["rotations"])
    return ro, out


def partial_tiles(H, W):
    """bool [tiles_y, tiles_x]: the tiles that are only partly inside the image."""
    part = np.zeros(((H + 15) // 16, (W + 15) // 16), bool)
    if W % 16:
        part[:, -1] = True
    if H % 16:
        part[-1, :] = True
    return part


def edge_rows(ro, H, W):
    """bool [P]: the visible Gaussians whose every tile instance (the oracle's 3-sigma lists) lies in a partial tile."""
    keys, vals, ranges, tt, nc = ro.binning()
    part = partial_tiles(H, W).reshape(-1)
    tile = (keys >> np.uint64(32)).astype(np.int64)
    rows = tt > 0
    rows[vals[~part[tile]]] = False
    return rows


def list_statistics(ro):
    """Per partial tile (y, x): the length of its list and the deepest and median n_contrib of its inside pixels."""
    keys, vals, ranges, tt, nc = ro.binning()
    H, W = ro.H, ro.W
    part = partial_tiles(H, W)
    length = (ranges[:, 1].astype(np.int64) - ranges[:, 0].astype(np.int64)).reshape(part.shape)
    out = {}
    for ty, tx in zip(*np.nonzero(part)):
        inside = nc[ty * 16:(ty + 1) * 16, tx * 16:(tx + 1) * 16]
        out["%d,%d" % (ty, tx)] = dict(entries=int(length[ty, tx]), pixels=int(inside.size), n_contrib_max=int(inside.max()),
                                       n_contrib_median=float(np.median(inside)))
    return out
