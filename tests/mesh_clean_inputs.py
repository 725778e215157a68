"""Seeded inputs of the mesh cleaning and decimation tests (tests/test_mesh_clean_cpu.py, tests/test_gpu_mesh_clean.py).  Everything is
(vertices [V, 3] float32, faces [F, 3] int32) in numpy."""
import numpy as np


def strip_piece(nfaces, origin, du, dv):
    """A triangle strip of `nfaces` faces: vertex j at origin + (j // 2) du + (j % 2) dv, face i = (i, i + 1, i + 2), every other one
    turned so that all face one way.  (vertices [nfaces + 2, 3] float64, faces [nfaces, 3] int64)."""
    j = np.arange(nfaces + 2)
    v = np.asarray(origin, np.float64)[None] + (j // 2)[:, None] * np.asarray(du, np.float64)[None] + (j % 2)[:, None] * np.asarray(dv, np.float64)[None]
    i = np.arange(nfaces)
    f = np.stack((i, np.where(i % 2 == 0, i + 1, i + 2), np.where(i % 2 == 0, i + 2, i + 1)), 1)
    return v, f


def join(pieces, extra_vertices=0, seed=None):
    """The pieces in one mesh; `extra_vertices` unreferenced vertices are mixed in; with a seed the vertex indices and the face order
    are permuted.  Also returns the piece of every face."""
    vs, fs, owner, base = [], [], [], 0
    for k, (v, f) in enumerate(pieces):
        vs.append(v)
        fs.append(f + base)
        owner.append(np.full(len(f), k))
        base += len(v)
    rng = np.random.default_rng(0 if seed is None else seed)
    if extra_vertices:
        vs.append(rng.uniform(-1, 1, (extra_vertices, 3)))
    v, f, owner = np.concatenate(vs), np.concatenate(fs), np.concatenate(owner)
    if seed is not None:
        perm = rng.permutation(len(v))            # old index -> new index
        out = np.empty_like(v)
        out[perm] = v
        order = rng.permutation(len(f))
        v, f, owner = out, perm[f][order], owner[order]
    return v.astype(np.float32), f.astype(np.int32), owner


def permuted_strip(V=4096, seed=3):
    """One strip over V vertices whose indices are randomly permuted: the minimum has to travel a long way."""
    v, f = strip_piece(V - 2, (0, 0, 0), (1.0 / V, 0, 0), (0, 0.01, 0))
    return join([(v, f)], seed=seed)[:2]


def strips(F, seed=5):
    """F faces in strips of at most 10, permuted."""
    pieces = [strip_piece(min(10, F - s), (0, 0.1 * (s // 10), 0), (0.01, 0, 0), (0, 0.02, 0)) for s in range(0, F, 10)]
    return join(pieces, seed=seed)[:2]


def mixed_components(seed=7):
    """Components of 1, 7, 8 and 500 faces and 9 unreferenced vertices, permuted."""
    pieces = [strip_piece(n, (0, 0.2 * k, 0), (0.01, 0, 0), (0, 0.05, 0)) for k, n in enumerate((1, 7, 8, 500))]
    return join(pieces, extra_vertices=9, seed=seed)


def special():
    """name -> (faces, V): a face with a repeated index, an edge shared by three faces, two blobs touching at one vertex, no face."""
    tetra = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]])
    return {
        "repeated_index": (np.array([[4, 4, 2], [0, 1, 3], [5, 6, 6]], np.int32), 8),
        "three_faces_one_edge": (np.array([[5, 1, 2], [1, 5, 3], [5, 1, 0], [6, 7, 8]], np.int32), 9),
        "touching_blobs": (np.concatenate((tetra + 3, np.where(tetra == 0, 3, tetra + 6), tetra + 10)).astype(np.int32), 14),
        "empty": (np.zeros((0, 3), np.int32), 5),
    }


# ---- clean_mesh.  The scene's box is about 1 x 1 x 0.4 (diagonal D about 1.5); pieces: 0 a 500-face sheet, 1 seven faces, 2 eight faces
# (both 0.2 long: 13 % of D), 3 eight faces long and thin (0.4 x 0.001: 27 % of D), 4 eight tiny faces (0.004 x 0.001: 0.3 % of D), 5 and
# 6 twenty faces each (the tie of keep_largest).  Nothing is within a factor of 2 of min_diameter = 0.05, let alone 1e-3.
CLEAN_PIECES = ("sheet", "seven", "eight", "thin", "tiny", "tie_a", "tie_b")


def clean_scene(seed=11):
    pieces = [strip_piece(500, (0, 0, 0), (0.004, 0, 0), (0, 1.0, 0.4)),
              strip_piece(7, (0.1, 0.1, 0.3), (0.05, 0, 0), (0, 0.05, 0)),
              strip_piece(8, (0.1, 0.3, 0.3), (0.04, 0, 0), (0, 0.05, 0)),
              strip_piece(8, (0.5, 0.5, 0.1), (0.1, 0, 0), (0, 0.001, 0)),
              strip_piece(8, (0.7, 0.7, 0.2), (0.001, 0, 0), (0, 0.001, 0)),
              strip_piece(20, (0.2, 0.6, 0.35), (0.02, 0, 0), (0, 0.03, 0)),
              strip_piece(20, (0.2, 0.8, 0.35), (0.02, 0, 0), (0, 0.03, 0))]
    return join(pieces, extra_vertices=5, seed=seed)


# ---- cluster_decimate
def dyadic_boundary(seed=13):
    """Vertices on multiples of 1 / 16 in [-0.5, 0.5]^3 with both corners of the box present: at n = 8 (h = 1 / 8) every second one lies
    exactly on a cell boundary, and the ones at 0.5 on the upper face of the box.  Float32 is exact on all of it."""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 17, (400, 3)) / 16.0 - 0.5
    v[0], v[1] = -0.5, 0.5
    v[2:20, 0] = 0.5
    v[20:40, 2] = 0.5
    f = rng.integers(0, 400, (900, 3))
    return v.astype(np.float32), f.astype(np.int32)


def flat_patch(seed=17, N=33):
    """An N x N sheet in the plane through `origin` spanned by two orthonormal vectors, its interior vertices jittered inside the plane;
    (vertices, faces, unit normal, origin)."""
    rng = np.random.default_rng(seed)
    e0 = np.array([2.0, 1.0, -1.0]) / np.sqrt(6.0)
    e1 = np.array([1.0, -1.0, 1.0]) / np.sqrt(3.0)
    normal = np.cross(e0, e1)
    i, j = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    uv = np.stack((i, j), -1).astype(np.float64)
    uv[1:-1, 1:-1] += rng.uniform(-0.3, 0.3, (N - 2, N - 2, 2))
    uv /= N - 1
    origin = np.array([0.3, -0.2, 0.1])
    v = origin + uv[..., :1] * e0 + uv[..., 1:] * e1
    idx = (i * N + j)
    a, b, c, d = idx[:-1, :-1], idx[1:, :-1], idx[:-1, 1:], idx[1:, 1:]
    f = np.concatenate((np.stack((a, b, c), -1).reshape(-1, 3), np.stack((c, b, d), -1).reshape(-1, 3)))
    return v.reshape(-1, 3).astype(np.float32), f.astype(np.int32), normal, origin


CUBE_GRID, CUBE_BOX = 13, 1.3          # 13 cells over [-1.3, 1.3]: h = 0.2, the cube's corners (+-1) at the centres of cells 1 and 11


def cube(steps=39):
    """The cube [-1, 1]^3, every face a steps x steps grid of squares, each square four triangles around its centre (so the tessellation
    has the cube's full symmetry), outward winding; two unreferenced vertices at +-1.3 widen the clustering grid so that every corner
    of the cube lies strictly inside a cell (CUBE_GRID).  With an odd `steps` no vertex lies on a cell boundary of that grid (the boundaries
    are at -0.9 + 0.2 j, the vertices at -1 + k / steps)."""
    t = np.linspace(-1, 1, steps + 1)
    table, verts, faces = {}, [], []

    def vid(p):
        key = tuple(np.round(np.asarray(p) * steps * 2).astype(np.int64))
        if key not in table:
            table[key] = len(verts)
            verts.append(np.asarray(p, np.float64))
        return table[key]

    for axis in range(3):
        for side in (-1.0, 1.0):
            u_ax, v_ax = (axis + 1) % 3, (axis + 2) % 3
            for i in range(steps):
                for j in range(steps):
                    def pt(u, v):
                        p = np.zeros(3)
                        p[axis], p[u_ax], p[v_ax] = side, u, v
                        return p
                    c00, c10, c11, c01 = (vid(pt(t[i], t[j])), vid(pt(t[i + 1], t[j])), vid(pt(t[i + 1], t[j + 1])), vid(pt(t[i], t[j + 1])))
                    mid = vid(pt((t[i] + t[i + 1]) / 2, (t[j] + t[j + 1]) / 2))
                    ring = (c00, c10, c11, c01) if side > 0 else (c01, c11, c10, c00)
                    for k in range(4):
                        faces.append((ring[k], ring[(k + 1) % 4], mid))
    verts += [np.full(3, -CUBE_BOX), np.full(3, CUBE_BOX)]
    return np.asarray(verts, np.float32), np.asarray(faces, np.int32)


def unit_cube():
    """The 12-face cube on 8 vertices."""
    v = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], np.float32)
    f = np.array([[0, 2, 1], [1, 2, 3], [4, 5, 6], [5, 7, 6], [0, 1, 4], [1, 5, 4], [2, 6, 3], [3, 6, 7], [0, 4, 2], [2, 4, 6], [1, 3, 5], [3, 7, 5]],
                 np.int32)
    return v, f
