"""The definitions of csrc/mesh_clean.hip and gaussianip_amd/utils/mesh.py (connected_components, clean_mesh, cluster_decimate,
decimate_mesh) restated in numpy, written from the definitions and not from the kernels.

Components are a union-find; `flood_fill` is the brute force it is checked against.  The grid is computed in float32 in the kernels'
operand order, so cell membership is comparable exactly; `cell_indices_exact` is the same in rational arithmetic, for inputs on which
float32 is exact.  The placement runs in a dtype of the caller's choice on the float32 membership: float64 is the reference, float32
(the same formulas, numpy's summation order) measures what float32 costs."""
from fractions import Fraction

import numpy as np

LAMBDA = 1e-3


# ---------------------------------------------------------------------------------------------------------------- components
def _valid(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(1)


def components(faces, V):
    """labels [V] int32: the smallest vertex index of every vertex's component (union-find, the smaller root wins)."""
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    f = np.asarray(faces, np.int64).reshape(-1, 3)
    for a, b, c in f[_valid(f, V)]:
        for x, y in ((a, b), (b, c)):
            rx, ry = find(int(x)), find(int(y))
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    return np.array([find(v) for v in range(V)], np.int32)


def flood_fill(faces, V):
    """The same labels by brute force: repeated sweeps over an adjacency matrix."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    adj = np.eye(V, dtype=bool)
    for a, b, c in f[_valid(f, V)]:
        for x, y in ((a, b), (b, c), (a, c)):
            adj[x, y] = adj[y, x] = True
    labels = np.full(V, -1, np.int64)
    for v in range(V):
        if labels[v] >= 0:
            continue
        seen = np.zeros(V, bool)
        seen[v] = True
        while True:
            grown = adj[seen].any(0)
            if (grown == seen).all():
                break
            seen = grown
        labels[seen] = v
    return labels.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- cleaning
def _sq(d):
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def clean(vertices, faces, min_faces=8, min_diameter=0.05, keep_largest=False, dtype=np.float32):
    """dict(vertices, faces, labels, vertex_map, face_map, num_components, num_kept, sq_diagonal {label: value}, bar): clean_mesh with
    the box arithmetic in `dtype`."""
    v = np.asarray(vertices, np.float32).astype(dtype)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(v)
    labels = components(f, V)
    ok = _valid(f, V)
    flab = np.where(ok, labels[np.clip(f[:, 0], 0, max(V - 1, 0))], -1)
    roots = np.unique(flab[ok])
    count = {int(r): int((flab == r).sum()) for r in roots}
    box = {}
    for r in roots:
        pts = v[f[flab == r].reshape(-1)]
        box[int(r)] = (pts.min(0), pts.max(0))
    sq = {r: _sq(box[r][1] - box[r][0]) for r in box}
    if box:
        whole = np.sqrt(_sq(np.max([b[1] for b in box.values()], 0) - np.min([b[0] for b in box.values()], 0)))
    else:
        whole = dtype(0)
    t = dtype(min_diameter) * whole
    bar = t * t
    kept = [r for r in sorted(box) if count[r] >= min_faces and sq[r] >= bar]
    if keep_largest and kept:
        kept = [max(kept, key=lambda r: (count[r], -r))]
    face_keep = np.isin(flab, kept) & ok
    used = np.zeros(V, bool)
    used[f[face_keep].reshape(-1)] = True
    vertex_map = np.where(used, np.cumsum(used) - 1, -1).astype(np.int32)
    return dict(vertices=np.asarray(vertices, np.float32)[used], faces=vertex_map[f[face_keep]].astype(np.int32).reshape(-1, 3), labels=labels,
                vertex_map=vertex_map, face_map=np.nonzero(face_keep)[0].astype(np.int32), num_components=len(box), num_kept=len(kept),
                sq_diagonal=sq, bar=bar, count=count)


# ---------------------------------------------------------------------------------------------------------------- the grid
def grid_frame(vertices, n):
    """(lo [3] float32, h float32): the per-axis minimum and L / n, L the largest extent, in float32."""
    v = np.asarray(vertices, np.float32)
    lo = v.min(0)
    L = np.float32((v.max(0) - lo).max())
    return lo, np.float32(L / np.float32(n))


def cell_indices(vertices, n):
    """(idx [V, 3] int64, keys [V] int64) in float32, the kernels' operand order: i = min((int) floor((p - lo) / h), n - 1)."""
    v = np.asarray(vertices, np.float32)
    lo, h = grid_frame(v, n)
    t = np.floor((v - lo[None]) / h)
    assert t.dtype == np.float32
    idx = np.minimum(np.maximum(t, 0).astype(np.int64), n - 1)
    return idx, (idx[:, 2] * n + idx[:, 1]) * n + idx[:, 0]


def cell_indices_exact(vertices, n):
    """The same in exact rational arithmetic (lo, L and h included): equal to cell_indices wherever float32 is exact."""
    v = [[Fraction(float(x)) for x in row] for row in np.asarray(vertices, np.float32)]
    lo = [min(r[a] for r in v) for a in range(3)]
    L = max(max(r[a] for r in v) - lo[a] for a in range(3))
    h = L / n
    idx = np.array([[min(int((r[a] - lo[a]) // h), n - 1) for a in range(3)] for r in v], np.int64)
    return idx, (idx[:, 2] * n + idx[:, 1]) * n + idx[:, 0]


def face_count(vertices, faces, n):
    """The faces whose three corners lie in three different cells."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = _valid(f, len(vertices))
    k = cell_indices(vertices, n)[1][f[ok]]
    return int(((k[:, 0] != k[:, 1]) & (k[:, 1] != k[:, 2]) & (k[:, 0] != k[:, 2])).sum())


# ---------------------------------------------------------------------------------------------------------------- clustering
def cluster(vertices, faces, n, dtype=np.float64):
    """dict(vertices [C', 3] dtype, faces [F', 3] int32, vertex_map [V] int32, all_vertices [C, 3] (every occupied cell, before the
    removal of unreferenced ones), mean [C, 3] (the members' mean, as a position), cell_of [V], cells [C, 3], new_id [C], lo, h)."""
    v32 = np.asarray(vertices, np.float32)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    V = len(v32)
    f = f[_valid(f, V)] if not _valid(f, V).all() else f
    idx, keys = cell_indices(v32, n)
    lo32, h32 = grid_frame(v32, n)
    cell_key, cell_of = np.unique(keys, return_inverse=True)
    C = len(cell_key)
    cells = np.stack((cell_key % n, (cell_key // n) % n, cell_key // (n * n)), 1)
    v, lo, h = v32.astype(dtype), lo32.astype(dtype), dtype(h32)
    centre = lo[None] + (cells.astype(dtype) + dtype(0.5)) * h                 # [C, 3]
    A = np.zeros((C, 6), dtype)
    b = np.zeros((C, 3), dtype)
    for k in range(3):
        cell = cell_of[f[:, k]]
        c = centre[cell]
        qa, qb, qc = ((v[f[:, j]] - c) / h for j in range(3))
        nrm = np.cross(qb - qa, qc - qa).astype(dtype)
        w = np.sqrt(nrm[:, 0] * nrm[:, 0] + nrm[:, 1] * nrm[:, 1] + nrm[:, 2] * nrm[:, 2])
        m = w > 0
        nrm, w, cell, qa = nrm[m], w[m], cell[m], qa[m]
        d = nrm[:, 0] * qa[:, 0] + nrm[:, 1] * qa[:, 1] + nrm[:, 2] * qa[:, 2]
        for slot, (i, j) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            np.add.at(A[:, slot], cell, (nrm[:, i] * nrm[:, j]) / w)
        for i in range(3):
            np.add.at(b[:, i], cell, (nrm[:, i] * d) / w)
    msum = np.zeros((C, 3), dtype)
    q = (v - centre[cell_of]) / h
    for i in range(3):
        np.add.at(msum[:, i], cell_of, q[:, i])
    mean = msum / np.bincount(cell_of, minlength=C).astype(dtype)[:, None]
    tr = A[:, 0] + A[:, 3] + A[:, 5]
    r = dtype(LAMBDA) * tr
    safe = np.where(tr > 0, r, dtype(1))
    a00, a01, a02, a11, a12, a22 = A[:, 0] + safe, A[:, 1], A[:, 2], A[:, 3] + safe, A[:, 4], A[:, 5] + safe
    r0, r1, r2 = (b[:, i] + r * mean[:, i] for i in range(3))
    l10, l20 = a01 / a00, a02 / a00
    d1 = a11 - l10 * a01
    t12 = a12 - l20 * a01
    l21 = t12 / d1
    d2 = a22 - l20 * a02 - l21 * t12
    y0, y1 = r0, r1 - l10 * r0
    y2 = r2 - l20 * y0 - l21 * y1
    z = y2 / d2
    y = y1 / d1 - l21 * z
    x = y0 / a00 - l10 * y - l20 * z
    sol = np.where((tr > 0)[:, None], np.stack((x, y, z), 1), mean)
    sol = np.clip(sol, dtype(-0.5), dtype(0.5))
    placed = centre + h * sol
    # faces
    nf = cell_of[f]
    alive = (nf[:, 0] != nf[:, 1]) & (nf[:, 1] != nf[:, 2]) & (nf[:, 0] != nf[:, 2])
    s = np.sort(nf, 1)
    packed = (s[:, 0] << 42) | (s[:, 1] << 21) | s[:, 2]
    keep = np.zeros(len(f), bool)
    if alive.any():
        cand = np.nonzero(alive)[0]
        _, first = np.unique(packed[cand], return_index=True)                  # the first occurrence: the lowest input index
        keep[cand[first]] = True
    used = np.zeros(C, bool)
    used[nf[keep].reshape(-1)] = True
    new_id = np.where(used, np.cumsum(used) - 1, -1).astype(np.int32)
    return dict(vertices=placed[used], faces=new_id[nf[keep]].reshape(-1, 3), vertex_map=new_id[cell_of], all_vertices=placed,
                mean=centre + h * np.clip(mean, dtype(-0.5), dtype(0.5)), cell_of=cell_of, cells=cells, new_id=new_id, lo=lo32, h=h32)
