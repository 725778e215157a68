"""A numpy restatement of the projection of rendered views onto the texture atlas, from its definition (the header of
gaussianip_amd/csrc/texture_project.hip), in float32 (the kernel's operand order) or float64; and of utils.texture.visible_depth from
the rasterizer's restatement (tests/mesh_render_reference.py).

project() also says, per texel, whether some decision of some view is within a margin of flipping: w near 0, sx or sy near an integer
(which covers the image border and the choice of the visibility pixel), the depth test, the min_cos test, the min_alpha test.  Only
decisions that the view reaches count: one taken with room to spare at an earlier step hides the later ones.  The flags are always
evaluated in float64, whatever `dtype` is."""
import numpy as np

import mesh_render_reference as mref
import texture_reference

# the margins inside which a decision counts as "could flip" (tests/texture_project_inputs.py records how they were fixed)
MARGIN_PX = 1e-4          # sx, sy: pixels
MARGIN = 2e-5             # w, cos: absolute; the depth test: relative to max(1, w)
MARGIN_ALPHA = 5e-5       # the looked-up alpha inherits the error of sx, sy through the bilinear weights: 2e-5 is less than 8 x 5.5e-6


def pack_views(projs, centres):
    """[K, 20] float32: full_proj_transform (row-major), camera centre, 0."""
    K = len(projs)
    out = np.zeros((K, 20), np.float32)
    out[:, :16] = np.asarray(projs, np.float32).reshape(K, 16)
    out[:, 16:19] = np.asarray(centres, np.float32).reshape(K, 3)
    return out


def clip_positions(vertices, projs):
    """[K, V, 4] float32: (v, 1) M in float32, what visible_depth rasterizes (a float32 matmul; its rounding is the rasterizer's input,
    so a test feeds the kernel's own positions to the restatement where bits matter)."""
    v = np.asarray(vertices, np.float32)
    vh = np.concatenate((v, np.ones((len(v), 1), np.float32)), 1)
    return np.stack([vh @ np.asarray(m, np.float32).reshape(4, 4) for m in projs]).astype(np.float32)


def visible_depth(pos, tri, H, W, dtype=np.float32):
    """[K, H, W]: the clip w of the surface visible at every pixel centre (0 where empty): the rasterizer's restatement, then w
    interpolated as an attribute, (u w0 + v w1) + ((1 - u) - v) w2."""
    ids = mref.rasterize(pos, tri, H, W)["tri"]
    u, v, _ = mref.barycentrics(pos, tri, H, W, ids, dtype)
    K = pos.shape[0]
    out = mref.interpolate(np.asarray(pos, np.float32)[..., 3:4], tri, ids, u, v, dtype)
    assert out.shape == (K, H, W, 1)
    return out[..., 0]


def _bilinear(img, x, y, dt):
    """img [H, W, 4] at (x, y) [N] (pixel-index coordinates), indices clamped."""
    H, W = img.shape[:2]
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = (x - xf)[:, None], (y - yf)[:, None]
    xi, yi = xf.astype(np.int64), yf.astype(np.int64)
    x0, x1, y0, y1 = np.clip(xi, 0, W - 1), np.clip(xi + 1, 0, W - 1), np.clip(yi, 0, H - 1), np.clip(yi + 1, 0, H - 1)
    one = dt(1)
    t = img.astype(dt)
    return (one - fy) * ((one - fx) * t[y0, x0] + fx * t[y0, x1]) + fy * ((one - fx) * t[y1, x0] + fx * t[y1, x1])


def _run(vertices, faces, T, views, images, vis_depth, depth_tolerance, min_cos, min_alpha, two_sided, unpremultiply, dt):
    """The definition in dtype dt over the owned texels.  Returns the sums and, per view, every quantity a decision is taken on."""
    faces = np.asarray(faces, np.int64)
    F = faces.shape[0]
    views = np.asarray(views, np.float32)
    K, H, W = vis_depth.shape
    p, f, x, y = texture_reference.points(vertices, faces, T, dt)
    v = np.asarray(vertices, np.float32).astype(dt)
    e1, e2 = v[faces[f, 1]] - v[faces[f, 0]], v[faces[f, 2]] - v[faces[f, 0]]
    n = np.stack((e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]), 1)
    nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    N = len(p)
    live = nn > 0
    color, weight, count = np.zeros((N, 3), dt), np.zeros(N, dt), np.zeros(N, np.int64)
    q = {k: np.zeros((K, N), dt) for k in ("w", "sx", "sy", "depth", "cos", "alpha")}
    reached = np.zeros((K, 6, N), bool)            # the view takes decision s: w, inside the image, depth, cos, alpha; [5]: it passes
    half, tol = dt(0.5), dt(np.float32(depth_tolerance))
    with np.errstate(all="ignore"):
        for k in range(K):
            m = views[k, :16].reshape(4, 4).astype(dt)
            cam = views[k, 16:19].astype(dt)
            col = lambda j: ((p[:, 0] * m[0, j] + p[:, 1] * m[1, j]) + p[:, 2] * m[2, j]) + m[3, j]  # noqa: E731
            w, cx, cy = col(3), col(0), col(1)
            ok = live.copy()
            reached[k, 0] = ok
            ok = ok & (w > 0)
            sx, sy = ((cx / w) * half + half) * dt(W), ((cy / w) * half + half) * dt(H)
            reached[k, 1] = ok
            ok = ok & (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
            ix, iy = np.where(ok, np.floor(sx), 0).astype(np.int64), np.where(ok, np.floor(sy), 0).astype(np.int64)
            wp = np.asarray(vis_depth, np.float32)[k, iy, ix].astype(dt)
            reached[k, 2] = ok & (wp > 0)              # an empty pixel is decided by the rasterizer, not here; sx, sy cover its choice
            ok = ok & (wp > 0) & ~(w - wp > tol)
            d = cam[None, :] - p
            dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            c = ((n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]) / (np.sqrt(nn) * np.sqrt(dd))
            if two_sided:
                c = np.abs(c)
            reached[k, 3] = ok
            ok = ok & (c >= dt(np.float32(min_cos)))
            tap = _bilinear(np.asarray(images, np.float32)[k], np.where(ok, sx - half, 0), np.where(ok, sy - half, 0), dt)
            al = tap[:, 3]
            reached[k, 4] = ok
            ok = ok & (al >= dt(np.float32(min_alpha)))
            reached[k, 5] = ok
            rgb = tap[:, :3] / al[:, None] if unpremultiply else tap[:, :3]
            wt = c * c
            weight = np.where(ok, weight + wt, weight)
            color = np.where(ok[:, None], color + wt[:, None] * rgb, color)
            count += ok
            for key, val in (("w", w), ("sx", sx), ("sy", sy), ("depth", (w - wp) - tol), ("cos", c), ("alpha", al)):
                q[key][k] = val
    assert color.dtype == dt and weight.dtype == dt
    return dict(color=color, weight=weight, count=count, q=q, reached=reached, x=x, y=y, face=f, live=live, H=H, W=W, own=texture_reference.owner(F, T)[0])


def _near_image(q, H, W):
    return (q["sx"] > -1) & (q["sx"] < W + 1) & (q["sy"] > -1) & (q["sy"] < H + 1)


def _flags(r, min_cos, min_alpha):
    """[N] bool from a float64 run: some reached decision of some view lies within its margin."""
    q, reached = r["q"], r["reached"]
    near_int = lambda s: np.abs(s - np.rint(s)) < MARGIN_PX  # noqa: E731
    with np.errstate(all="ignore"):
        flag = reached[:, 0] & (np.abs(q["w"]) < MARGIN)
        flag |= reached[:, 1] & (q["w"] > 0) & _near_image(q, r["H"], r["W"]) & (near_int(q["sx"]) | near_int(q["sy"]))
        flag |= reached[:, 2] & (np.abs(q["depth"]) / np.maximum(1, q["w"]) < MARGIN)
        flag |= reached[:, 3] & (np.abs(q["cos"] - np.float64(np.float32(min_cos))) < MARGIN)
        flag |= reached[:, 4] & (np.abs(q["alpha"] - np.float64(np.float32(min_alpha))) < MARGIN_ALPHA)
    return flag.any(0)


def project(vertices, faces, T, views, images, vis_depth, depth_tolerance, min_cos=0.2, min_alpha=0.5, two_sided=True, unpremultiply=False,
            dtype=np.float64):
    """{"color_sum": [T, T, 3], "weight_sum": [T, T], "count": [T, T] int64, "owned", "flagged": [T, T] bool, ...} of the definition in
    `dtype`: vertices [V, 3] world, faces [F, 3], views [K, 20] (pack_views), images [K, H, W, 4] interleaved float32, vis_depth
    [K, H, W] float32.  "flagged" comes from a float64 evaluation.  "run": the per-view quantities over the owned texels (row-major order)
    and the float64 run as "run64"."""
    args = (vertices, faces, T, views, images, np.asarray(vis_depth, np.float32), depth_tolerance, min_cos, min_alpha, two_sided, unpremultiply)
    r64 = _run(*args, np.float64)
    r = r64 if dtype == np.float64 else _run(*args, dtype)
    y, x = r["y"], r["x"]
    color, weight, count = np.zeros((T, T, 3), dtype), np.zeros((T, T), dtype), np.zeros((T, T), np.int64)
    flagged, owned = np.zeros((T, T), bool), r["own"] >= 0
    color[y, x], weight[y, x], count[y, x] = r["color"], r["weight"], r["count"]
    flagged[y, x] = _flags(r64, min_cos, min_alpha)
    return dict(color_sum=color, weight_sum=weight, count=count, owned=owned, flagged=flagged, run=r, run64=r64)


def deviations(r32, r64):
    """{"w", "px", "depth", "cos", "alpha"}: the largest float32 - float64 deviation of every decision quantity, in the units of its
    margin, over the decisions the float64 run reaches (sx and sy: where the projection lies within a pixel of the image)."""
    q32, q64, reached = r32["q"], r64["q"], r64["reached"]

    def worst(keys, mask, scale=None):
        out = 0.0
        for key in keys:
            d = np.abs(q32[key].astype(np.float64) - q64[key])
            d = (d if scale is None else d / scale)[mask]
            d = d[np.isfinite(d)]
            out = max(out, float(d.max()) if d.size else 0.0)
        return out
    with np.errstate(all="ignore"):
        near = reached[:, 1] & (q64["w"] > 0) & _near_image(q64, r64["H"], r64["W"])
        return dict(w=worst(("w",), reached[:, 0]), px=worst(("sx", "sy"), near), depth=worst(("depth",), reached[:, 2], np.maximum(1, q64["w"])),
                    cos=worst(("cos",), reached[:, 3]), alpha=worst(("alpha",), reached[:, 4]))
