"""The seeded meshes of the geometry-term tests (tests/golden/mesh_geometry.npz holds the reference's values on them; pure numpy).

icosphere(level): the icosahedron subdivided `level` times on the unit sphere, 10 * 4^level + 2 vertices and 20 * 4^level faces; the
four children of a face are consecutive, so the last faces of the list lie next to each other on the sphere.

mesh(name) -> (v [V, 3] float32, f [F, 3] int32, w [V, 3] float32, tags):
  "a"  level 2 (V 164, F 305), "b"  level 4 plus a fan (V 2635, F 5175).  Both: the sphere scaled by (1.0, 0.8, 1.3), every vertex moved
  by seeded noise whose root-mean-square length is a fifth of the mean edge length, the last 17 faces removed (a boundary; the vertices
  that only they named stay in the list, unreferenced), then
    one face with a repeated index (a, a, b) on an existing edge: its pair (a, a) is an edge of the reference's Mesh.edges,
    one isolated vertex, appended (it takes the default normal, like the unreferenced ones),
    one extra face on an existing interior edge with a new third vertex: three faces share that edge.
  "b" also gets a closed fan of 70 faces around one apex with 70 rim vertices, above the sphere: a row of the corner table and of the
  neighbour table that is longer than a wave.
  w is the seeded weight of the normals' gradient, d(sum w . n) / dv.  tags: the indices the tests name."""
import functools
import os

import numpy as np

SCALE = np.array([1.0, 0.8, 1.3])
REMOVED, FAN = 17, 70
SPECS = {"a": dict(level=2, seed=11, fan=False), "b": dict(level=4, seed=12, fan=True)}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mesh_geometry.npz")
QUANTITIES = ("v_nrm", "lap", "nc", "g_nrm", "g_lap", "g_nc")


def icosphere(level):
    """(v [V, 3] float64 on the unit sphere, f [F, 3] int64)."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], np.int64)
    for _ in range(level):
        V = v.shape[0]
        a, b, c = f[:, 0], f[:, 1], f[:, 2]
        ends = np.stack((np.concatenate((a, b, c)), np.concatenate((b, c, a))), 1)
        key = ends.min(1) * V + ends.max(1)
        uniq, inv = np.unique(key, return_inverse=True)
        mid = v[uniq // V] + v[uniq % V]
        v = np.concatenate((v, mid / np.linalg.norm(mid, axis=1, keepdims=True)))
        F = f.shape[0]
        inv = inv.reshape(-1)
        ab, bc, ca = V + inv[:F], V + inv[F:2 * F], V + inv[2 * F:]
        f = np.stack((np.stack((a, ab, ca), 1), np.stack((b, bc, ab), 1), np.stack((c, ca, bc), 1), np.stack((ab, bc, ca), 1)), 1).reshape(-1, 3)
    return v, f


def mean_edge_length(v, f):
    e = np.concatenate((v[f[:, 0]] - v[f[:, 1]], v[f[:, 1]] - v[f[:, 2]], v[f[:, 2]] - v[f[:, 0]]))
    return float(np.linalg.norm(e, axis=1).mean())


@functools.lru_cache(maxsize=None)
def _mesh(name):
    spec = SPECS[name]
    rng = np.random.default_rng(spec["seed"])
    v, f = icosphere(spec["level"])
    v = v * SCALE
    edge = mean_edge_length(v, f)
    v = v + rng.normal(size=v.shape) * (0.2 * edge / 3.0 ** 0.5)
    f = f[:-REMOVED]
    V0 = v.shape[0]
    a, b = int(f[0, 0]), int(f[0, 1])
    repeated = np.array([[a, a, b]])
    isolated = np.array([[0.1, -0.2, 0.15]])
    p, q = int(f[7, 1]), int(f[7, 2])                      # an interior edge: two faces have it already
    wing = (v[p] + v[q]) * 0.5 * 1.25 + rng.normal(size=3) * (0.2 * edge)
    v = np.concatenate((v, isolated, wing[None]))
    f = np.concatenate((f, repeated, [[q, p, V0 + 1]]))
    tags = dict(repeated_face=f.shape[0] - 2, self_pair=(a, a), isolated=V0, wing=V0 + 1, three_face_edge=(min(p, q), max(p, q)))
    if spec["fan"]:
        apex, rim0 = v.shape[0], v.shape[0] + 1
        ang = 2.0 * np.pi * np.arange(FAN) / FAN
        rim = np.stack((0.5 * np.cos(ang), 0.5 * np.sin(ang), np.full(FAN, 2.0)), 1) + rng.normal(size=(FAN, 3)) * 0.008
        v = np.concatenate((v, [[0.0, 0.0, 2.3]], rim))
        i = np.arange(FAN)
        f = np.concatenate((f, np.stack((np.full(FAN, apex), rim0 + i, rim0 + (i + 1) % FAN), 1)))
        tags.update(apex=apex, rim=(rim0, rim0 + FAN))
    w = rng.normal(size=v.shape)
    referenced = np.zeros(v.shape[0], bool)
    referenced[f.reshape(-1)] = True
    tags["unreferenced"] = tuple(int(i) for i in np.nonzero(~referenced)[0])
    return v.astype(np.float32), f.astype(np.int32), w.astype(np.float32), tags


def mesh(name):
    v, f, w, tags = _mesh(name)
    return v.copy(), f.copy(), w.copy(), dict(tags)


@functools.lru_cache(maxsize=None)
def load_golden():
    """The fixture as a dictionary of arrays (read-only by convention: the tests share it)."""
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
