"""A numpy restatement of pixel differentials and the mipmapped lookup from their definition (the header of
gaussianip_amd/csrc/mesh_mip.hip), in the manner of tests/mesh_render_reference.py: float32 in the kernel's operand order, or float64.
The triangle set-up (snapping, integer edge functions) and the bilinear rule are mesh_render_reference's."""
import numpy as np

import mesh_render_reference as ref

F32 = np.float32
LN2 = 0.69314718055994530942


# ---------------------------------------------------------------------------------------------------------------- rast_db
def _slopes(s, dtype):
    """(dXb, dYb): the derivatives of the three screen-space weights in the pixel, from the integer set-up s."""
    x0, y0, x1, y1, x2, y2, area = s
    sg = -1 if area < 0 else 1
    fa = dtype(sg * area)
    dx = [dtype(-256 * sg * (y2 - y1)) / fa, dtype(-256 * sg * (y0 - y2)) / fa, dtype(-256 * sg * (y1 - y0)) / fa]
    dy = [dtype(256 * sg * (x2 - x1)) / fa, dtype(256 * sg * (x0 - x2)) / fa, dtype(256 * sg * (x1 - x0)) / fa]
    return dx, dy


def rast_db(pos, tri, H, W, ids, u, v, dtype):
    """[B, H, W, 4] = (du/dX, du/dY, dv/dX, dv/dY) in `dtype` for the triangle ids names at every pixel (zeros where ids < 0); u, v
    [B, H, W] are what rast holds (mesh_render_reference.barycentrics in the same dtype)."""
    pos = np.asarray(pos, F32)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    B = pos.shape[0]
    out = np.zeros((B, H, W, 4), dtype)
    u, v = u.astype(dtype), v.astype(dtype)
    for b in range(B):
        X, Y, ok = ref.snap(pos[b], H, W)
        p = pos[b].astype(dtype)
        for f in np.unique(ids[b]):
            if f < 0:
                continue
            t = tri[f]
            s = ref._setup(X, Y, ok, t)
            py, px = np.nonzero(ids[b] == f)
            e0, e1, e2, area = ref._edges(s, 256 * px.astype(np.int64) + 128, 256 * py.astype(np.int64) + 128)
            fa = dtype(area)
            w0, w1, w2 = p[t[0], 3], p[t[1], 3], p[t[2], 3]
            q0, q1, q2 = (e0.astype(dtype) / fa) / w0, (e1.astype(dtype) / fa) / w1, (e2.astype(dtype) / fa) / w2
            S = (q0 + q1) + q2
            dx, dy = _slopes(s, dtype)
            uu, vv = u[b, py, px], v[b, py, px]
            for k, d in enumerate((dx, dy)):
                dq0, dq1, dq2 = d[0] / w0, d[1] / w1, d[2] / w2
                dS = (dq0 + dq1) + dq2
                out[b, py, px, k] = (dq0 - uu * dS) / S
                out[b, py, px, 2 + k] = (dq1 - vv * dS) / S
    return out


def uv_at(pos_view, t, H, W, point):
    """(u, v) in float64 of triangle t = (i0, i1, i2) of one view at the continuous pixel position point = (X, Y) (pixel (px, py) has
    its centre at X = px, Y = py): the definition's weights with the integer edge functions evaluated at a real point."""
    X, Y, ok = ref.snap(np.asarray(pos_view, F32), H, W)
    s = ref._setup(X, Y, ok, t)
    Px, Py = 256.0 * point[0] + 128.0, 256.0 * point[1] + 128.0
    e0, e1, e2, area = ref._edges(s, Px, Py)
    w = np.asarray(pos_view, np.float64)[list(t), 3]
    q0, q1, q2 = e0 / area / w[0], e1 / area / w[1], e2 / area / w[2]
    S = (q0 + q1) + q2
    return np.array([q0 / S, q1 / S])


# ---------------------------------------------------------------------------------------------------------------- attribute differentials
def _rows(attr, idx, ids, dtype):
    a = np.asarray(attr).astype(dtype)
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    B = ids.shape[0]
    rows = idx[np.maximum(ids, 0)]                                  # [B, H, W, 3]
    pick = (lambda k: np.stack([a[b][rows[b, ..., k]] for b in range(B)])) if a.ndim == 3 else (lambda k: a[rows[..., k]])
    return pick(0), pick(1), pick(2), rows


def interpolate_da(attr, idx, ids, db, channels, dtype):
    """[B, H, W, 2 K]: (da/dX, da/dY) of the listed channels (None: all) of attr [N, C] or [B, N, C]; db = rast_db; 0 where empty."""
    a0, a1, a2, _ = _rows(attr, idx, ids, dtype)
    ch = list(range(a0.shape[-1])) if channels is None else list(channels)
    db = db.astype(dtype)
    d0, d1 = (a0 - a2)[..., ch], (a1 - a2)[..., ch]
    dX = db[..., 0:1] * d0 + db[..., 2:3] * d1
    dY = db[..., 1:2] * d0 + db[..., 3:4] * d1
    out = np.stack((dX, dY), -1).reshape(ids.shape + (2 * len(ch),))
    return np.where((ids >= 0)[..., None], out, dtype(0))


def interpolate_da_grad(shape, idx, ids, db, channels, g, dtype):
    """dL/dattr (of `shape`: [N, C] shared by the views, or [B, N, C]) of sum(g * interpolate_da(attr, ...)), analytically."""
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    C = shape[-1]
    ch = list(range(C)) if channels is None else list(channels)
    db = db.astype(dtype)
    g = np.asarray(g).astype(dtype).reshape(ids.shape + (len(ch), 2))
    g0 = db[..., 0:1] * g[..., 0] + db[..., 1:2] * g[..., 1]
    g1 = db[..., 2:3] * g[..., 0] + db[..., 3:4] * g[..., 1]
    out = np.zeros(shape, dtype)
    for b in range(ids.shape[0]):
        m = ids[b] >= 0
        rows = idx[ids[b][m]]
        dst = out[b] if len(shape) == 3 else out
        for k, gk in enumerate((g0[b][m], g1[b][m], -(g0[b][m] + g1[b][m]))):
            for j, c in enumerate(ch):
                np.add.at(dst[:, c], rows[:, k], gk[:, j])
    return out


# ---------------------------------------------------------------------------------------------------------------- the mip stack
def mip_levels(Th, Tw, max_level=None):
    """L, the index of the last level."""
    L, h, w = 0, Th, Tw
    while (h > 1 or w > 1) and (max_level is None or L < max_level) and (h == 1 or h % 2 == 0) and (w == 1 or w % 2 == 0):
        h, w, L = max(h // 2, 1), max(w // 2, 1), L + 1
    return L


def _down(t, dtype):
    h, w = t.shape[:2]
    if h > 1 and w > 1:
        return ((t[0::2, 0::2] + t[0::2, 1::2]) + (t[1::2, 0::2] + t[1::2, 1::2])) * dtype(0.25)
    if h > 1:
        return (t[0::2] + t[1::2]) * dtype(0.5)
    return (t[:, 0::2] + t[:, 1::2]) * dtype(0.5)


def mip_build(tex, max_level, dtype):
    """The levels 0 .. L of tex [Th, Tw, C] as a list."""
    levels = [np.asarray(tex).astype(dtype)]
    for _ in range(mip_levels(levels[0].shape[0], levels[0].shape[1], max_level)):
        levels.append(_down(levels[-1], dtype))
    return levels


def mip_fold(grads, dtype):
    """The gradient stack (a list like mip_build's) folded to level 0 top-down: the transpose of the build."""
    g = [np.array(x, dtype) for x in grads]
    for l in range(len(g) - 2, -1, -1):
        h, w = g[l].shape[:2]
        up = g[l + 1]
        if h > 1:
            up = np.repeat(up, 2, 0)
        if w > 1:
            up = np.repeat(up, 2, 1)
        g[l] = g[l] + dtype(0.25 if (h > 1 and w > 1) else 0.5) * up
    return g[0]


# ---------------------------------------------------------------------------------------------------------------- the lookup
def lod(uv_da, bias, Th, Tw, shape, dtype):
    """The level before the clamp and the intermediate values of its chain, for pixels of `shape`; uv_da and bias may be None."""
    r = {k: np.zeros(shape, dtype) for k in ("sx", "sy", "tx", "ty", "D", "Cc", "R", "m")}
    level = np.zeros(shape, dtype) if bias is None else np.asarray(bias).astype(dtype)
    if uv_da is not None:
        d = np.asarray(uv_da).astype(dtype)
        sx, sy, tx, ty = d[..., 0] * dtype(Tw), d[..., 1] * dtype(Tw), d[..., 2] * dtype(Th), d[..., 3] * dtype(Th)
        A, B = sx * sx + tx * tx, sy * sy + ty * ty
        Cc = sx * sy + tx * ty
        D = A - B
        R = np.sqrt(dtype(0.25) * (D * D) + Cc * Cc)
        m = dtype(0.5) * (A + B) + R
        with np.errstate(all="ignore"):
            level = dtype(0.5) * np.log2(m) + level
        r.update(sx=sx, sy=sy, tx=tx, ty=ty, D=D, Cc=Cc, R=R, m=m)
    r["level"] = level.astype(dtype)
    return r


def select(level, L, nearest, dtype):
    """(l0, l1 int64, f) of the clamped level."""
    lc = np.minimum(np.maximum(np.where(np.isnan(level), dtype(0), level), dtype(0)), dtype(L)).astype(dtype)
    if nearest:
        l0 = np.minimum(np.floor(lc + dtype(0.5)).astype(np.int64), L)
        return l0, l0.copy(), np.zeros(lc.shape, dtype)
    fl = np.floor(lc)
    l0 = np.clip(fl.astype(np.int64), 0, L)
    return l0, np.minimum(l0 + 1, L), (lc - fl).astype(dtype)


def _bil_all(levels, uv, dtype):
    return [ref.texture(t, uv, dtype) for t in levels]


def texture_mip(levels, uv, uv_da, bias, dtype, nearest=False):
    """[..., C]: the mipmapped lookup of the stack `levels` (mip_build's list) at uv [..., 2]."""
    levels = [np.asarray(t).astype(dtype) for t in levels]
    L = len(levels) - 1
    uv = np.asarray(uv)
    l0, l1, f = select(lod(uv_da, bias, levels[0].shape[0], levels[0].shape[1], uv.shape[:-1], dtype)["level"], L, nearest, dtype)
    bil = _bil_all(levels, uv, dtype)
    v0 = sum(np.where((l0 == l)[..., None], bil[l], dtype(0)) for l in range(L + 1))
    v1 = sum(np.where((l1 == l)[..., None], bil[l], dtype(0)) for l in range(L + 1))
    f = f[..., None]
    return np.where(f == 0, v0, (dtype(1) - f) * v0 + f * v1).astype(dtype)


def texture_mip_grad(levels, uv, uv_da, bias, g, dtype, nearest=False):
    """(dL/dtex [Th, Tw, C] (folded), dL/duv [..., 2], dL/duv_da [..., 4], dL/dbias [...], the texels of level 0 whose 2^l x 2^l block
    a footprint reaches: bool [Th, Tw]) of sum(g * texture_mip(...)), analytically.  The last two gradients are those of the
    definition whether or not uv_da / bias were given (zeros for an absent uv_da)."""
    levels = [np.asarray(t).astype(dtype) for t in levels]
    L = len(levels) - 1
    Th, Tw = levels[0].shape[:2]
    uv = np.asarray(uv)
    shape = uv.shape[:-1]
    r = lod(uv_da, bias, Th, Tw, shape, dtype)
    level = r["level"]
    l0, l1, f = select(level, L, nearest, dtype)
    g = np.asarray(g).astype(dtype)
    one = dtype(1)
    gv0, gv1 = (one - f)[..., None] * g, f[..., None] * g
    with np.errstate(invalid="ignore"):
        gate = (level > 0) & (level < L) & (not nearest)
    g_uv = np.zeros(shape + (2,), dtype)
    stack, reached = [], []
    for l, t in enumerate(levels):
        m0, m1 = l0 == l, (l1 == l) & (f != 0)
        gt0, guv0 = ref.texture_grad(t, uv, gv0, m0, dtype)
        gt1, guv1 = ref.texture_grad(t, uv, gv1, m1, dtype)
        stack.append(gt0 + gt1)
        g_uv = g_uv + (guv0 + guv1)
        x0, x1, y0, y1, _, _ = ref.lookup_setup(uv, t.shape[0], t.shape[1], dtype)
        hit = np.zeros(t.shape[:2], bool)
        for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)):
            hit[yy[m0 | m1], xx[m0 | m1]] = True
        reached.append(hit)
    bil = _bil_all(levels, uv, dtype)
    lhi = np.minimum(l0 + 1, L)
    v0 = sum(np.where((l0 == l)[..., None], bil[l], dtype(0)) for l in range(L + 1))
    v1 = sum(np.where((lhi == l)[..., None], bil[l], dtype(0)) for l in range(L + 1))
    dl = np.where(gate, (g * (v1 - v0)).sum(-1), dtype(0)).astype(dtype)
    g_da = np.zeros(shape + (4,), dtype)
    if uv_da is not None:
        with np.errstate(all="ignore"):
            k = dl * dtype(0.5) / (r["m"] * dtype(LN2))
            e = np.where(r["R"] > 0, dtype(0.25) * r["D"] / r["R"], dtype(0))
            mA, mB = dtype(0.5) + e, dtype(0.5) - e
            mC = np.where(r["R"] > 0, r["Cc"] / r["R"], dtype(0))
            two = dtype(2)
            parts = ((mA * (two * r["sx"]) + mC * r["sy"]) * dtype(Tw), (mB * (two * r["sy"]) + mC * r["sx"]) * dtype(Tw),
                     (mA * (two * r["tx"]) + mC * r["ty"]) * dtype(Th), (mB * (two * r["ty"]) + mC * r["tx"]) * dtype(Th))
            ok = gate & (r["m"] > 0)
            g_da = np.stack([np.where(ok, k * p, dtype(0)) for p in parts], -1).astype(dtype)
    # a level-l texel stands for its 2^l x 2^l block of level 0 (2^l x 1 where a side has run out)
    touched = np.zeros((Th, Tw), bool)
    for l, hit in enumerate(reached):
        touched |= np.repeat(np.repeat(hit, Th // hit.shape[0], 0), Tw // hit.shape[1], 1)
    return mip_fold(stack, dtype), g_uv, g_da, dl, touched
