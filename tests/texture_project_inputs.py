"""Seeded scenes of the view-projection tests (tests/test_texture_project_cpu.py, tests/test_gpu_texture_project.py): a mesh in world
coordinates, K pinhole cameras as (full_proj_transform, camera centre), K random images with alpha, and the visibility depth of every
view from the rasterizer's restatement.  Everything is numpy; nothing here needs a GPU.

The cameras are built here and not by scene.Camera, so that the CPU tests need no torch: eye, target and a vertical field of view
give the row-vector matrix M with clip = (p, 1) M, clip w = the distance along the optical axis (so depth_tolerance is in world units),
clip x / w and y / w in [-1, 1] across the image, and z / w in [0, 1] between the near and the far plane.

The margins (tests/texture_project_reference.py) were fixed by the rule "at least 8 times the largest deviation of the quantity between
the float32 and the float64 restatement on these scenes", starting from 1e-4 pixels for sx, sy and 2e-5 for the others.  MEASURED below
holds the deviations over all scenes and flag combinations (test_texture_project_cpu.py::test_margins_cover_the_float32_error measures
them again, prints them and asserts the rule).  Four of the five starting margins hold; the looked-up alpha deviates by 5.4e-6 (it
inherits the 1e-5 pixels of sx, sy through the bilinear weights), so its margin is 5e-5."""
import functools

import numpy as np

import mesh_render_inputs
import sample_inputs
import texture_inputs

H, W = mesh_render_inputs.H, mesh_render_inputs.W      # 45 x 67
PARITY_SIZE = 64
DEGENERATE = 7            # the face of the parity scene whose three vertices coincide
ZNEAR, ZFAR = 0.01, 100.0
FLAG_CAP = 0.02           # at most this share of the owned texels may be flagged in any scene

# The largest float32 - float64 deviations measured on the scenes below, in the margins' units (w, cos, alpha absolute; px pixels;
# depth relative to max(1, w)); 8 times each must stay below the margin.
MEASURED = {"w": 2.2e-7, "px": 9.6e-6, "depth": 9.3e-8, "cos": 2.2e-7, "alpha": 5.5e-6}


def camera(eye, target, fovy_deg, h, w, up=(0.0, 1.0, 0.0)):
    """(M [4, 4] float32, centre [3] float32) of a pinhole camera at `eye` looking at `target`."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    f = target - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, np.asarray(up, np.float64))
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    ty = np.tan(np.radians(fovy_deg) / 2)
    tx = ty * w / h
    M = np.zeros((4, 4), np.float64)
    for j, (axis, s) in enumerate(((r, 1 / tx), (u, 1 / ty))):
        M[:3, j], M[3, j] = axis * s, -np.dot(axis, eye) * s
    a = ZFAR / (ZFAR - ZNEAR)
    M[:3, 2], M[3, 2] = f * a, -np.dot(f, eye) * a - ZNEAR * a
    M[:3, 3], M[3, 3] = f, -np.dot(f, eye)
    return M.astype(np.float32), eye.astype(np.float32)


def _images(K, h, w, seed):
    """[K, h, w, 4] float32: random colours and alphas in [0, 1]."""
    return np.random.default_rng(seed).uniform(0, 1, (K, h, w, 4)).astype(np.float32)


def _finish(vertices, faces, T, cams, images, tol, extra=None, h=H, w=W):
    """The scene dict.  extra: {view: (vertices, faces)} of occluders that only the visibility of that view sees."""
    import texture_project_reference as ref
    projs, centres = [c[0] for c in cams], [c[1] for c in cams]
    pos = ref.clip_positions(vertices, projs)
    vis = ref.visible_depth(pos, faces, h, w)
    for k, (ov, of) in (extra or {}).items():
        allv, allf = np.concatenate((vertices, ov)), np.concatenate((faces, of + len(vertices)))
        vis[k] = ref.visible_depth(ref.clip_positions(allv, projs[k:k + 1]), allf, h, w)[0]
    return dict(vertices=vertices, faces=faces, T=T, projs=np.stack(projs), centres=np.stack(centres), views=ref.pack_views(projs, centres),
                images=images, vis_depth=np.ascontiguousarray(vis, np.float32), depth_tolerance=tol, H=h, W=w, K=len(cams))


@functools.lru_cache(maxsize=None)
def parity_scene():
    """sphere_mesh(F = 40) at T = 64 (cell 12), three cameras at 67 x 45: one outside that sees the whole sphere, with a sheet in front
    of half of it; one with a narrow field of view aimed past the sphere, so that part of it is off-screen; one INSIDE the sphere,
    so that half of the faces lie behind it (w <= 0).  Face DEGENERATE is collapsed to a point."""
    v, f = texture_inputs.sphere_mesh(40)
    v = v.copy()
    v[f[DEGENERATE]] = v[f[DEGENERATE, 0]]
    mu, rad = sample_inputs.SPHERE_MU, sample_inputs.SPHERE_RADIUS
    cams = [camera(mu + np.array([0.1, 0.2, 1.2]), mu, 25.0, H, W),
            camera(mu + np.array([0.9, 0.25, -0.3]), mu + np.array([0.0, 0.12, 0.1]), 14.0, H, W),
            camera(mu + np.array([0.02, -0.03, 0.01]), mu + np.array([0.3, 1.0, 0.2]), 100.0, H, W)]
    # the sheet: two triangles between camera 0 and the sphere, covering x < mu_x + 0.03
    z = mu[2] + 2.5 * rad
    sheet = np.array([[mu[0] - 1.0, mu[1] - 1.0, z], [mu[0] + 0.03, mu[1] - 1.0, z], [mu[0] + 0.03, mu[1] + 1.0, z], [mu[0] - 1.0, mu[1] + 1.0, z]],
                     np.float32)
    quad = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    return _finish(v, f, PARITY_SIZE, cams, _images(3, H, W, 11), 0.02, extra={0: (sheet, quad)})


def _orbit(K, seed, fovy, h, w, dist=2.5, jitter=0.0):
    rng = np.random.default_rng(seed)
    cams = []
    for k in range(K):
        az = 2 * np.pi * k / max(K, 1) + 0.3
        eye = dist * np.array([np.cos(az) * 0.9, 0.35, np.sin(az) * 0.9]) + rng.uniform(-jitter, jitter, 3)
        cams.append(camera(eye, rng.uniform(-jitter, jitter, 3), fovy, h, w))
    return cams


EXTREMES = ("F1_T16_K1", "F2_T16_K3", "F128_T32_K64", "F7_T21_K3")


@functools.lru_cache(maxsize=None)
def extreme_scene(name):
    """F = 1 and F = 2 at T = 16 (one cell of side 16), F = 128 at T = 32 (cell 4: the atlas is full) under 64 jittered copies of
    four cameras at 16 x 12, and a texture side that is no power of two (T = 21, cell 10, one unowned column and row)."""
    F, T, K = (int(s[1:]) for s in name.split("_"))
    v, f = texture_inputs.random_mesh(F, seed=300 + F, extent=0.5, half_extent=0.12)
    if K == 64:
        h, w = 12, 16
        rng = np.random.default_rng(5)
        base = _orbit(4, 6, 14.0, h, w)
        cams = []
        for k in range(K):      # a narrow field of view aimed at a random point: every view sees a part of the mesh only
            eye = base[k % 4][1].astype(np.float64) + rng.uniform(-0.2, 0.2, 3)
            cams.append(camera(eye, rng.uniform(-0.5, 0.5, 3), 14.0, h, w))
    else:
        h, w = H, W
        cams = _orbit(K, 7 + F, 35.0, h, w, jitter=0.1)
    return _finish(v, f, T, cams, _images(K, h, w, 20 + F), 0.05, h=h, w=w)


def all_scenes():
    return [("parity", parity_scene())] + [(n, extreme_scene(n)) for n in EXTREMES]


FLAG_COMBINATIONS = [(True, False), (True, True), (False, False), (False, True)]      # (two_sided, unpremultiply)


# ---------------------------------------------------------------------------------------------------------------- round trip
RAMP = np.array([[0.011, 0.003, 0.1], [0.002, 0.013, 0.05], [-0.006, 0.004, 0.6]])      # per channel (a, b, c0): a sx + b sy + c0
PLANE_W = 2.0
PLANE_SIZE = 384          # cells of side 54: a texel step is under a third of a pixel, so the footprint of a pixel one away from the border stays unclamped


def plane_scene(h=H, w=W):
    """(world vertices [63, 3] float32, faces [96, 3]): the jittered grid of the rasterizer tests flattened onto the plane w = PLANE_W,
    perpendicular to the optical axis of mesh_render_inputs.EXACT_PROJ's camera (clip = (x, y, 0.5, z) exactly): screen coordinates are
    an affine function of the surface point, so a linear ramp in pixel coordinates is linear on the surface.  Every vertex is moved to
    the nearest point of the rasterizer's sub-pixel grid (1 / 256 pixel), so that the triangles it rasterizes are the triangles
    themselves and the surface point of a pixel is its centre; otherwise the snapping alone would move it by up to 0.002 pixels."""
    pos, tri = mesh_render_inputs.grid_mesh(1000, h=h, w=w)
    ndc = pos[:, :2].astype(np.float64) / pos[:, 3:4].astype(np.float64)
    screen = np.rint((ndc * 0.5 + 0.5) * np.array([w, h]) * 256) / 256
    ndc = screen / np.array([w, h]) * 2 - 1
    world = np.concatenate((ndc * PLANE_W, np.full((len(pos), 1), PLANE_W)), 1).astype(np.float32)
    return world, tri


def ramp_image(h=H, w=W):
    """[h, w, 4] float32: channel c is a sx + b sy + c0 at the pixel centre (sx, sy) = (ix + 0.5, iy + 0.5); alpha 1."""
    sy, sx = np.meshgrid(np.arange(h) + 0.5, np.arange(w) + 0.5, indexing="ij")
    img = np.ones((h, w, 4), np.float64)
    for c, (a, b, c0) in enumerate(RAMP):
        img[..., c] = a * sx + b * sy + c0
    return img.astype(np.float32)
