"""A numpy restatement of the mesh rasterizer from its definition (the header of gaussianip_amd/csrc/mesh_raster.hip).

Snapping is always float32, because it is the definition; coverage and the visibility key are exact integers; depth is float32 in the
stated order.  Barycentrics, interpolation, lookup and gradients run in float32 (the kernel's operand order) or in float64."""
import numpy as np

GUARD = 1 << 22
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
F32 = np.float32


def snap(pos, H, W):
    """(X, Y int64 [.., V], ok bool [.., V]) of clip-space pos [.., V, 4] float32: 8 sub-pixel bits; ok: w > 0 and inside the guard band."""
    pos = np.asarray(pos, F32)
    x, y, w = pos[..., 0], pos[..., 1], pos[..., 3]
    with np.errstate(all="ignore"):
        tx = np.rint(((x / w) * F32(0.5) + F32(0.5)) * F32(W) * F32(256.0))
        ty = np.rint(((y / w) * F32(0.5) + F32(0.5)) * F32(H) * F32(256.0))
        ok = (w > 0) & (np.abs(tx) <= GUARD) & (np.abs(ty) <= GUARD)
    X = np.where(ok, tx, 0).astype(np.int64)
    Y = np.where(ok, ty, 0).astype(np.int64)
    return X, Y, ok


def _owns(dx, dy):
    return (dy < 0) | ((dy == 0) & (dx > 0))


def _setup(X, Y, ok, t):
    """The integer set-up of triangle t = (i0, i1, i2) of one view, or None when it is dropped whole (culling aside)."""
    i0, i1, i2 = (int(i) for i in t)
    if not (ok[i0] and ok[i1] and ok[i2]):
        return None
    x0, y0, x1, y1, x2, y2 = int(X[i0]), int(Y[i0]), int(X[i1]), int(Y[i1]), int(X[i2]), int(Y[i2])
    area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
    if area == 0:
        return None
    return x0, y0, x1, y1, x2, y2, area


def _edges(s, Px, Py):
    """The normalised edge functions (int64 arrays) at the points (Px, Py) and the normalised area."""
    x0, y0, x1, y1, x2, y2, area = s
    sg = -1 if area < 0 else 1
    e0 = sg * ((x2 - x1) * (Py - y1) - (y2 - y1) * (Px - x1))
    e1 = sg * ((x0 - x2) * (Py - y2) - (y0 - y2) * (Px - x2))
    e2 = sg * ((x1 - x0) * (Py - y0) - (y1 - y0) * (Px - x0))
    return e0, e1, e2, sg * area


def _inside(s, e0, e1, e2):
    x0, y0, x1, y1, x2, y2, area = s
    sg = -1 if area < 0 else 1
    out = np.ones(e0.shape, bool)
    for e, (dx, dy) in ((e0, (x2 - x1, y2 - y1)), (e1, (x0 - x2, y0 - y2)), (e2, (x1 - x0, y1 - y0))):
        out &= (e > 0) | ((e == 0) & bool(_owns(np.int64(sg * dx), np.int64(sg * dy))))
    return out


def depth_key(d):
    """The order-preserving 32-bit image of float32 depths, as uint64."""
    u = np.ascontiguousarray(d, F32).view(np.uint32).copy()
    u[(u & np.uint32(0x7FFFFFFF)) == 0] = 0
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint64)


def rasterize(pos, tri, H, W, cull_backfaces=False):
    """{"tri": [B, H, W] int64 (-1: empty), "depth": [B, H, W] float32 (0 where empty), "covering": [B, H, W] the number of triangles
    whose coverage holds the pixel, depth test aside}."""
    pos = np.asarray(pos, F32)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    B, V = pos.shape[:2]
    keys = np.full((B, H, W), EMPTY, np.uint64)
    covering = np.zeros((B, H, W), np.int64)
    for b in range(B):
        X, Y, ok = snap(pos[b], H, W)
        with np.errstate(all="ignore"):
            zw = pos[b, :, 2] / pos[b, :, 3]
        for f, t in enumerate(tri):
            if t.min() < 0 or t.max() >= V:
                continue
            s = _setup(X, Y, ok, t)
            if s is None or (cull_backfaces and s[6] < 0):
                continue
            xs, ys = (s[0], s[2], s[4]), (s[1], s[3], s[5])
            x_lo, x_hi = max((min(xs) + 127) >> 8, 0), min((max(xs) - 128) >> 8, W - 1)
            y_lo, y_hi = max((min(ys) + 127) >> 8, 0), min((max(ys) - 128) >> 8, H - 1)
            if x_lo > x_hi or y_lo > y_hi:
                continue
            px, py = np.meshgrid(np.arange(x_lo, x_hi + 1, dtype=np.int64), np.arange(y_lo, y_hi + 1, dtype=np.int64))
            e0, e1, e2, area = _edges(s, 256 * px + 128, 256 * py + 128)
            inside = _inside(s, e0, e1, e2)
            if not inside.any():
                continue
            px, py, e0, e1, e2 = px[inside], py[inside], e0[inside], e1[inside], e2[inside]
            covering[b, py, px] += 1
            fa = F32(area)
            b0, b1, b2 = e0.astype(F32) / fa, e1.astype(F32) / fa, e2.astype(F32) / fa
            with np.errstate(all="ignore"):
                d = b0 * zw[t[0]] + b1 * zw[t[1]] + b2 * zw[t[2]]
                keep = (d >= -1) & (d <= 1)
            key = (depth_key(d) << np.uint64(32)) | np.uint64(f)
            px, py, key = px[keep], py[keep], key[keep]
            keys[b, py, px] = np.minimum(keys[b, py, px], key)      # a triangle holds a pixel once: no repeated index
    empty = keys == EMPTY
    u = (keys >> np.uint64(32)).astype(np.uint32)
    bits = np.where((u & np.uint32(0x80000000)) != 0, u ^ np.uint32(0x80000000), ~u)
    depth = np.where(empty, F32(0), bits.view(F32))
    ids = np.where(empty, -1, (keys & np.uint64(0xFFFFFFFF)).astype(np.int64))
    return {"tri": ids, "depth": depth.astype(F32), "covering": covering}


def barycentrics(pos, tri, H, W, ids, dtype, perspective=True):
    """(u, v, d) [B, H, W] in `dtype` of the triangle that ids [B, H, W] names at every pixel (zeros where ids < 0): the screen-space
    weights from the exact edge functions, then the perspective-correct u, v and the depth.  perspective=False: u, v are the
    screen-space weights themselves (what a rasterizer without perspective correction would interpolate with)."""
    pos = np.asarray(pos, F32)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    B = pos.shape[0]
    out = np.zeros((3, B, H, W), dtype)
    for b in range(B):
        X, Y, ok = snap(pos[b], H, W)
        p = pos[b].astype(dtype)
        for f in np.unique(ids[b]):
            if f < 0:
                continue
            t = tri[f]
            s = _setup(X, Y, ok, t)
            py, px = np.nonzero(ids[b] == f)
            e0, e1, e2, area = _edges(s, 256 * px.astype(np.int64) + 128, 256 * py.astype(np.int64) + 128)
            fa = dtype(area)
            b0, b1, b2 = e0.astype(dtype) / fa, e1.astype(dtype) / fa, e2.astype(dtype) / fa
            w0, w1, w2 = p[t[0], 3], p[t[1], 3], p[t[2], 3]
            q0, q1, q2 = (b0 / w0, b1 / w1, b2 / w2) if perspective else (b0, b1, b2)
            den = (q0 + q1) + q2
            out[0, b, py, px] = q0 / den
            out[1, b, py, px] = q1 / den
            out[2, b, py, px] = b0 * (p[t[0], 2] / w0) + b1 * (p[t[1], 2] / w1) + b2 * (p[t[2], 2] / w2)
    return out[0], out[1], out[2]


def interpolate(attr, idx, ids, u, v, dtype):
    """[B, H, W, C]: attr [N, C] (or [B, N, C]) at the rows idx[f] of the named triangle, (u a0 + v a1) + ((1 - u) - v) a2; 0 where empty."""
    a = np.asarray(attr).astype(dtype)
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    u, v = u.astype(dtype), v.astype(dtype)
    B = ids.shape[0]
    rows = idx[np.maximum(ids, 0)]                                  # [B, H, W, 3]
    pick = (lambda k: np.stack([a[b][rows[b, ..., k]] for b in range(B)])) if a.ndim == 3 else (lambda k: a[rows[..., k]])
    w = (dtype(1) - u) - v
    out = (u[..., None] * pick(0) + v[..., None] * pick(1)) + w[..., None] * pick(2)
    return np.where((ids >= 0)[..., None], out, dtype(0))


def lookup_setup(uv, Th, Tw, dtype):
    """(x0, x1, y0, y1 clamped int64, fx, fy) of the bilinear lookup at uv [..., 2]; uv (0, 0) is the corner of tex[0, 0]."""
    uv = np.asarray(uv).astype(dtype)
    x, y = uv[..., 0] * dtype(Tw) - dtype(0.5), uv[..., 1] * dtype(Th) - dtype(0.5)
    xf, yf = np.floor(x), np.floor(y)
    fx, fy = x - xf, y - yf
    xi, yi = np.clip(xf, -1, Tw).astype(np.int64), np.clip(yf, -1, Th).astype(np.int64)
    c = lambda i, n: np.clip(i, 0, n - 1)  # noqa: E731
    return c(xi, Tw), c(xi + 1, Tw), c(yi, Th), c(yi + 1, Th), fx, fy


def texture(tex, uv, dtype):
    """[..., C]: the bilinear lookup of tex [Th, Tw, C] at uv [..., 2]."""
    t = np.asarray(tex).astype(dtype)
    x0, x1, y0, y1, fx, fy = lookup_setup(uv, t.shape[0], t.shape[1], dtype)
    fx, fy = fx[..., None], fy[..., None]
    one = dtype(1)
    return (one - fy) * ((one - fx) * t[y0, x0] + fx * t[y0, x1]) + fy * ((one - fx) * t[y1, x0] + fx * t[y1, x1])


def texture_grad(tex, uv, g, mask, dtype):
    """(dL/dtex [Th, Tw, C], dL/duv [..., 2]) of sum(g * texture(tex, uv)) over the pixels of `mask`, analytically."""
    t = np.asarray(tex).astype(dtype)
    Th, Tw = t.shape[:2]
    x0, x1, y0, y1, fx, fy = lookup_setup(uv, Th, Tw, dtype)
    g = np.where(mask[..., None], np.asarray(g).astype(dtype), dtype(0))
    fx, fy = fx[..., None], fy[..., None]
    one = dtype(1)
    gt = np.zeros_like(t)
    np.add.at(gt, (y0, x0), (one - fy) * (one - fx) * g)
    np.add.at(gt, (y0, x1), (one - fy) * fx * g)
    np.add.at(gt, (y1, x0), fy * (one - fx) * g)
    np.add.at(gt, (y1, x1), fy * fx * g)
    gs = (g * ((one - fy) * (t[y0, x1] - t[y0, x0]) + fy * (t[y1, x1] - t[y1, x0]))).sum(-1) * dtype(Tw)
    gv = (g * ((one - fx) * (t[y1, x0] - t[y0, x0]) + fx * (t[y1, x1] - t[y0, x1]))).sum(-1) * dtype(Th)
    return gt, np.stack((gs, gv), -1)


def interpolate_grad(shape, idx, ids, u, v, g, dtype):
    """dL/dattr [N, C] of sum(g * interpolate(attr, ...)) (one attr for all views), analytically."""
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    u, v = u.astype(dtype), v.astype(dtype)
    w = (dtype(1) - u) - v
    g = np.asarray(g).astype(dtype)
    out = np.zeros(shape, dtype)
    m = ids >= 0
    rows = idx[ids[m]]
    for k, wk in enumerate((u, v, w)):
        np.add.at(out, rows[:, k], wk[m][:, None] * g[m])
    return out


def shade(tex, uv_faces, ids, u, v, bg, dtype):
    """(colour [B, H, W, 3], alpha [B, H, W]) of the fused shade: face-varying uv [F, 3, 2] (internal convention), texture [Th, Tw, 3]."""
    F = np.asarray(uv_faces).shape[0]
    st = interpolate(np.asarray(uv_faces).reshape(F * 3, 2), np.arange(F * 3).reshape(F, 3), ids, u, v, dtype)
    col = texture(tex, st, dtype)
    hit = ids >= 0
    return np.where(hit[..., None], col, np.asarray(bg).astype(dtype)), hit.astype(dtype)
