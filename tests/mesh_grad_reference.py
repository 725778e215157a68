"""A numpy restatement of gaussianip_amd/csrc/mesh_grad.hip from its header: the gradient of rast to clip-space positions, the gradients
of interpolated values to rast, edge topology by brute force, and the antialias pass with its gradients.

Every decision (which triangle, which pixel is near, which edge is a silhouette, whether it crosses) is taken in exact integers of the
snapped coordinates, as tests/mesh_render_reference.py takes coverage.  The arithmetic after that runs in float32 (the kernel's operand
order) or float64.  snapped=False replaces the snapped screen coordinates X / 256 by the float64 values (x / w * 0.5 + 0.5) * W they
stand for, with the decisions unchanged: the function the straight-through gradient differentiates, which central differences can
check."""
import numpy as np

import mesh_render_reference as ref

F32 = np.float32


def screen(pos, H, W, dtype, snapped=True):
    """(sx, sy) [.., V] in pixels: X / 256 of the snap, or the unrounded float64 value."""
    if snapped:
        X, Y, _ = ref.snap(pos, H, W)
        return X.astype(dtype) / dtype(256), Y.astype(dtype) / dtype(256)
    p = np.asarray(pos, np.float64)
    return (p[..., 0] / p[..., 3] * 0.5 + 0.5) * W, (p[..., 1] / p[..., 3] * 0.5 + 0.5) * H


def _weights(pos_b, t, px, py, H, W, dtype, snapped):
    """(b [3, n], n_x [3], n_y [3]) of triangle t at the pixels (px, py): the screen-space weights and their gradient in the pixel centre,
    in pixels."""
    if snapped:
        X, Y, ok = ref.snap(pos_b, H, W)
        s = ref._setup(X, Y, ok, t)
        e0, e1, e2, area = ref._edges(s, 256 * px.astype(np.int64) + 128, 256 * py.astype(np.int64) + 128)
        fa = dtype(area)
        b = np.stack((e0.astype(dtype) / fa, e1.astype(dtype) / fa, e2.astype(dtype) / fa))
        x0, y0, x1, y1, x2, y2, signed = s
        sc = dtype(256) * dtype(1 if signed > 0 else -1) / fa
        nx = np.array([y1 - y2, y2 - y0, y0 - y1]).astype(dtype) * sc
        ny = np.array([x2 - x1, x0 - x2, x1 - x0]).astype(dtype) * sc
        return b, nx, ny
    sx, sy = screen(pos_b, H, W, dtype, False)
    (x0, x1, x2), (y0, y1, y2) = sx[t], sy[t]
    cx, cy = px + 0.5, py + 0.5
    area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
    b = np.stack(((x2 - x1) * (cy - y1) - (y2 - y1) * (cx - x1), (x0 - x2) * (cy - y2) - (y0 - y2) * (cx - x2),
                  (x1 - x0) * (cy - y0) - (y1 - y0) * (cx - x0))) / area
    return b, np.array([y1 - y2, y2 - y0, y0 - y1]) / area, np.array([x2 - x1, x0 - x2, x1 - x0]) / area


def rasterize_values(pos, tri, H, W, ids, dtype=np.float64, snapped=False):
    """(u, v, d) [B, H, W] of the triangles ids names, from the screen coordinates of `snapped`: what rasterize_grad differentiates."""
    pos = np.asarray(pos)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    out = np.zeros((3,) + ids.shape, dtype)
    for b in range(ids.shape[0]):
        p = pos[b].astype(dtype)
        for f in np.unique(ids[b]):
            if f < 0:
                continue
            t = tri[f]
            py, px = np.nonzero(ids[b] == f)
            bw, _, _ = _weights(pos[b], t, px, py, H, W, dtype, snapped)
            w, z = p[t, 3], p[t, 2]
            q = bw / w[:, None]
            S = (q[0] + q[1]) + q[2]
            out[0, b, py, px], out[1, b, py, px] = q[0] / S, q[1] / S
            out[2, b, py, px] = bw[0] * (z[0] / w[0]) + bw[1] * (z[1] / w[1]) + bw[2] * (z[2] / w[2])
    return out[0], out[1], out[2]


def _to_clip(g_pos_b, i, p, gsx, gsy, gz, gw, H, W, dtype):
    """mg_add of the kernel file: dL/d(sx, sy) plus direct dL/dz, dL/dw of vertex i, summed into g_pos_b [V, 4]."""
    ax, ay = gsx * (dtype(0.5) * dtype(W)), gsy * (dtype(0.5) * dtype(H))
    g_pos_b[i, 0] += np.sum(ax / p[3], dtype=dtype)
    g_pos_b[i, 1] += np.sum(ay / p[3], dtype=dtype)
    g_pos_b[i, 2] += np.sum(gz, dtype=dtype)
    g_pos_b[i, 3] += np.sum(gw - (ax * (p[0] / p[3]) + ay * (p[1] / p[3])) / p[3], dtype=dtype)


def rasterize_grad(pos, tri, H, W, ids, g_rast, dtype, snapped=True):
    """dL/dpos [B, V, 4] of sum(g_rast[..., :3] * (u, v, d)) with the triangle at every pixel held fixed."""
    pos = np.asarray(pos)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    g_rast = np.asarray(g_rast).astype(dtype)
    g_pos = np.zeros(pos.shape, dtype)
    for b in range(ids.shape[0]):
        p = pos[b].astype(dtype)
        for f in np.unique(ids[b]):
            if f < 0:
                continue
            t = tri[f]
            py, px = np.nonzero(ids[b] == f)
            bw, nx, ny = _weights(pos[b], t, px, py, H, W, dtype, snapped)
            gu, gv, gd = (g_rast[b, py, px, c] for c in range(3))
            w, zw = p[t, 3], p[t, 2] / p[t, 3]
            q = bw / w[:, None]
            S = (q[0] + q[1]) + q[2]
            u, v = q[0] / S, q[1] / S
            k = gu * u + gv * v
            gq = ((gu - k) / S, (gv - k) / S, -k / S)
            gb = [gq[i] / w[i] + gd * zw[i] for i in range(3)]
            Gx = ((gb[0] * nx[0] + gb[1] * nx[1]) + gb[2] * nx[2])
            Gy = ((gb[0] * ny[0] + gb[1] * ny[1]) + gb[2] * ny[2])
            for i in range(3):
                _to_clip(g_pos[b], t[i], p[t[i]], -bw[i] * Gx, -bw[i] * Gy, gd * bw[i] / w[i],
                         -(gq[i] * q[i] + gd * bw[i] * zw[i]) / w[i], H, W, dtype)
    return g_pos


def interpolate_grad_rast(attr, idx, ids, g, dtype):
    """[B, H, W, 4] = (g_u, g_v, 0, 0) of sum(g * interpolate(attr, ...)): attr [N, C] or [B, N, C], g [B, H, W, C]."""
    a = np.asarray(attr).astype(dtype)
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    g = np.asarray(g).astype(dtype)
    B = ids.shape[0]
    rows = idx[np.maximum(ids, 0)]
    pick = (lambda k: np.stack([a[b][rows[b, ..., k]] for b in range(B)])) if a.ndim == 3 else (lambda k: a[rows[..., k]])
    a2 = pick(2)
    out = np.zeros(ids.shape + (4,), dtype)
    out[..., 0] = (g * (pick(0) - a2)).sum(-1)
    out[..., 1] = (g * (pick(1) - a2)).sum(-1)
    return np.where((ids >= 0)[..., None], out, dtype(0))


def shade_grad_rast(tex, uv_faces, ids, u, v, g, dtype):
    """[B, H, W, 4] = (g_u, g_v, 0, 0) of sum(g * colour) of the fused shade: uv_faces [F, 3, 2] in the internal (flipped) convention."""
    F = np.asarray(uv_faces).shape[0]
    flat, corner = np.asarray(uv_faces).reshape(F * 3, 2), np.arange(F * 3).reshape(F, 3)
    st = ref.interpolate(flat, corner, ids, u, v, dtype)
    _, g_st = ref.texture_grad(tex, st, g, ids >= 0, dtype)
    return interpolate_grad_rast(flat, corner, ids, g_st, dtype)


# ------------------------------------------------------------------------------------------------------------------ topology
def edge_topology(tri):
    """[F, 3] by counting: for edge k (opposite corner k) of face f, the opposite vertex of the one other face with that edge, -1 when
    there is none, -2 when there are several."""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    out = np.zeros(tri.shape, np.int32)
    for f, t in enumerate(tri):
        for k in range(3):
            e = {t[(k + 1) % 3], t[(k + 2) % 3]}
            found = [(g, j) for g, s in enumerate(tri) for j in range(3) if (g, j) != (f, k) and {s[(j + 1) % 3], s[(j + 2) % 3]} == e]
            out[f, k] = -1 if not found else (-2 if len(found) > 1 else tri[found[0][0], found[0][1]])
    return out


# ------------------------------------------------------------------------------------------------------------------ antialias
def _orient(xp, yp, xq, yq, xr, yr):
    return (xq - xp) * (yr - yp) - (yq - yp) * (xr - xp)


def antialias_hits(pos, tri, topo, ids, depth, H, W):
    """The pairs that blend, from integers alone: a list of dicts with b, near and other (y, x), axis (0: horizontal), s, iP, iQ, and
    the integers n, D (tau = n / D), Cn, Cr.  ids [B, H, W] (-1: empty) and depth [B, H, W] are rast's."""
    pos = np.asarray(pos, F32)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    hits = []
    for b in range(ids.shape[0]):
        X, Y, ok = ref.snap(pos[b], H, W)
        X, Y = [int(v) for v in X], [int(v) for v in Y]
        for axis, (dy, dx) in enumerate(((0, 1), (1, 0))):
            A, C = (X, Y) if axis == 0 else (Y, X)          # along and across the pair's axis
            ya, xa = np.nonzero(ids[b, :H - dy, :W - dx] != ids[b, dy:, dx:])
            for y, x in zip(ya.tolist(), xa.tolist()):
                a, o = (y, x), (y + dy, x + dx)
                ia, ib = int(ids[b][a]), int(ids[b][o])
                da, db = depth[b][a], depth[b][o]
                n_is_a = ia >= 0 and (ib < 0 or da < db or (da == db and ia < ib))
                near, other = (a, o) if n_is_a else (o, a)
                f = int(ids[b][near])
                t = [int(i) for i in tri[f]]
                if ref._setup(np.array(X), np.array(Y), ok, t) is None:
                    continue
                s = 1 if n_is_a else -1
                Cn, Cr = 256 * near[1 - axis] + 128, 256 * near[axis] + 128
                for k in range(3):
                    iP, iQ, iR = t[(k + 1) % 3], t[(k + 2) % 3], t[k]
                    if (C[iP] > Cr) == (C[iQ] > Cr):
                        continue
                    D = C[iQ] - C[iP]
                    n = s * ((A[iP] - Cn) * D + (A[iQ] - A[iP]) * (Cr - C[iP]))
                    if D < 0:
                        D, n = -D, -n
                    if n < 0 or n > 256 * D:
                        continue
                    nb = int(topo[f, k])
                    if nb != -1:
                        if nb < 0 or nb >= pos.shape[1]:
                            continue
                        if ok[nb]:
                            o1 = _orient(X[iP], Y[iP], X[iQ], Y[iQ], X[iR], Y[iR])
                            o2 = _orient(X[iP], Y[iP], X[iQ], Y[iQ], X[nb], Y[nb])
                            if (o1 > 0 and o2 < 0) or (o1 < 0 and o2 > 0):
                                continue
                    hits.append(dict(b=b, near=near, other=other, axis=axis, s=s, iP=iP, iQ=iQ, n=n, D=D, Cn=Cn, Cr=Cr, face=f, edge=k))
                    break
    return hits


def _crossing(h, pos, H, W, dtype, snapped):
    """(t, lambda, m) of a hit."""
    if snapped:
        X, Y, _ = ref.snap(pos[h["b"]], H, W)
        A, C = (X, Y) if h["axis"] == 0 else (Y, X)
        cq_cp = dtype(int(C[h["iQ"]] - C[h["iP"]]))
        return ((dtype(h["n"]) / dtype(h["D"])) / dtype(256), dtype(int(h["Cr"] - C[h["iP"]])) / cq_cp,
                dtype(int(A[h["iQ"]] - A[h["iP"]])) / cq_cp)
    sx, sy = screen(pos[h["b"]], H, W, dtype, False)
    A, C = (sx, sy) if h["axis"] == 0 else (sy, sx)
    aP, aQ, cP, cQ = A[h["iP"]], A[h["iQ"]], C[h["iP"]], C[h["iQ"]]
    lam = (h["Cr"] / 256 - cP) / (cQ - cP)
    return h["s"] * (aP + (aQ - aP) * lam - h["Cn"] / 256), lam, (aQ - aP) / (cQ - cP)


def _blends(hits, pos, H, W, dtype, snapped):
    """Per hit that blends: (order key, hit, target, source, alpha, lambda, m), sorted so that every target's contributions come in the
    gather's order left, right, up, down."""
    out = []
    for h in hits:
        t, lam, m = _crossing(h, pos, H, W, dtype, snapped)
        half = dtype(0.5)
        # snapped: the side is the float comparison the kernel makes; otherwise it is one of the decisions, held as the integers took it
        side = int(t > half) - int(t < half) if snapped else int(2 * h["n"] > 256 * h["D"]) - int(2 * h["n"] < 256 * h["D"])
        if side > 0:
            target, source, alpha = h["other"], h["near"], t - half
        elif side < 0:
            target, source, alpha = h["near"], h["other"], half - t
        else:
            continue
        dy, dx = source[0] - target[0], source[1] - target[1]
        order = {(0, -1): 0, (0, 1): 1, (-1, 0): 2, (1, 0): 3}[(dy, dx)]
        out.append(((h["b"],) + target + (order,), h, target, source, alpha, lam, m))
    out.sort(key=lambda e: e[0])
    return out


def antialias(color, hits, pos, H, W, dtype, snapped=True):
    """out [B, H, W, C]."""
    color = np.asarray(color).astype(dtype)
    out = color.copy()
    for _, h, target, source, alpha, _, _ in _blends(hits, pos, H, W, dtype, snapped):
        b = h["b"]
        out[(b,) + target] = out[(b,) + target] + alpha * (color[(b,) + source] - color[(b,) + target])
    return out


def antialias_grad(color, hits, pos, g_out, H, W, dtype, snapped=True):
    """(dL/dcolor [B, H, W, C], dL/dpos [B, V, 4]) of sum(g_out * antialias(color, ...)), the decisions held fixed."""
    color, g_out = np.asarray(color).astype(dtype), np.asarray(g_out).astype(dtype)
    pos = np.asarray(pos)
    g_color, g_pos = g_out.copy(), np.zeros(pos.shape, dtype)
    for _, h, target, source, alpha, lam, m in _blends(hits, pos, H, W, dtype, snapped):
        b = h["b"]
        gt = g_out[(b,) + target]
        g_color[(b,) + target] -= alpha * gt
        g_color[(b,) + source] += alpha * gt
        dt = (gt * (color[(b,) + h["near"]] - color[(b,) + h["other"]])).sum(dtype=dtype)
        s = dtype(h["s"])
        along = (dt * s * (dtype(1) - lam), dt * s * lam)
        for i, al in zip((h["iP"], h["iQ"]), along):
            ac = -(al * m)
            gsx, gsy = (al, ac) if h["axis"] == 0 else (ac, al)
            _to_clip(g_pos[b], i, pos[b, i].astype(dtype), gsx, gsy, dtype(0), dtype(0), H, W, dtype)
    return g_color, g_pos
