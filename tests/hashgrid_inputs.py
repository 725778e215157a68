"""Seeded inputs of the hash-grid tests (tests/test_hashgrid_cpu.py, tests/test_gpu_hashgrid.py).  Every case is small enough for
seconds on the GPU and chosen where the kernels can still go wrong:
  a            L 6, F 2, 2^10 rows a level, base 4, scale 1.5, N 1000: three dense levels (64, 216, 736 rows) and three hashed ones
               (1024 rows for up to 29 791 nodes), so heavy collisions on both sides of the switch.
  b_f<F>_n<N>  the same with F 1, 4 and 8 at N 63 and 65: every row width, and a partial wave on either side of 64.
  c            the reference's default configuration (L 16, F 2, 2^19, base 16, scale 1.447269237440378) at N 257.
  d            edge points in configuration a: coordinates exactly 0, exactly 1 and exactly on grid nodes (frac == 0), 64 copies of
               one point (every lane scatters to the same rows), coordinates at -0.25 and 1.5, a NaN, an infinity and 1e12.
  e_n1, e_n0   one point, and none.
A case is (config, x [N, 3], table [P, F], g [N, L F]), all float32; the table is uniform in [-1, 1], g is normal."""
import functools

import numpy as np

CONFIG_A = {"otype": "HashGrid", "n_levels": 6, "n_features_per_level": 2, "log2_hashmap_size": 10, "base_resolution": 4,
            "per_level_scale": 1.5}
CONFIG_DEFAULT = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
                  "per_level_scale": 1.447269237440378}
CONFIG_SMALL = {"otype": "HashGrid", "n_levels": 8, "n_features_per_level": 2, "log2_hashmap_size": 14, "base_resolution": 8,
                "per_level_scale": 1.447269237440378}
CASES = ("a", "b_f1_n63", "b_f1_n65", "b_f4_n63", "b_f4_n65", "b_f8_n63", "b_f8_n65", "c", "d", "e_n1", "e_n0")
COPIES, COPIED_POINT = 64, (0.3125, 0.71, 0.052)
# rows of case d, in order
D_ZERO, D_ONE, D_NODES, D_COPIES, D_OUTSIDE, D_NONFINITE = slice(0, 4), slice(4, 8), slice(8, 20), slice(20, 84), slice(84, 90), slice(90, 96)


def config(name):
    if name == "c":
        return dict(CONFIG_DEFAULT)
    cfg = dict(CONFIG_A)
    if name.startswith("b_"):
        cfg["n_features_per_level"] = int(name.split("_")[1][1:])
    return cfg


def layout(name):
    from gaussianip_amd.utils.encoding import HashGridLayout
    return HashGridLayout(config(name))


def _edge_points(lay):
    rng = np.random.default_rng(40)
    zero = np.array([[0, 0, 0], [0, 0.37, 0.81], [0.6, 0, 0.2], [0.45, 0.9, 0]], np.float32)
    one = np.array([[1, 1, 1], [1, 0.37, 0.81], [0.6, 1, 0.2], [0.45, 0.9, 1]], np.float32)
    # on the nodes of a level: pos = x * scale + 0.5 is an integer, so x = (j - 0.5) / scale; 0.5 is one of them on level 0 (scale 3)
    nodes = [[0.5, 0.5, 0.5]]
    for l in (0, 1, 2, 3, 4):
        s = float(lay.scales[l])
        for _ in range(2):
            j = rng.integers(1, lay.resolutions[l], 3)
            nodes.append(((j - 0.5) / s).tolist())
    nodes.append([0.5, 0.25, 0.75])
    nodes = np.asarray(nodes, np.float32)
    copies = np.tile(np.asarray(COPIED_POINT, np.float32), (COPIES, 1))
    outside = np.array([[-0.25, 0.5, 0.5], [0.3, -0.25, 1.5], [1.5, 1.5, 1.5], [-0.25, -0.25, -0.25], [0.2, 0.4, 1.5], [1.5, 0.1, -0.25]],
                       np.float32)
    bad = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, 1e12], [-np.inf, 0.1, 0.2], [0.3, np.nan, np.inf], [1e12, -1e12, 0.5]],
                   np.float32)
    x = np.concatenate((zero, one, nodes, copies, outside, bad))
    assert x.shape[0] == D_NONFINITE.stop and nodes.shape[0] == D_NODES.stop - D_NODES.start
    return x


@functools.lru_cache(maxsize=None)
def case(name):
    """(config, x, table, g) of a case; the arrays are shared between the tests and must not be written to."""
    assert name in CASES, name
    cfg, lay = config(name), layout(name)
    rng = np.random.default_rng(1000 + CASES.index(name))
    if name == "d":
        x = _edge_points(lay)
    else:
        N = {"a": 1000, "c": 257, "e_n1": 1, "e_n0": 0}.get(name) if not name.startswith("b_") else int(name.split("_n")[1])
        x = rng.random((N, 3), dtype=np.float32)
    table = (rng.random((lay.n_rows, lay.n_features_per_level), dtype=np.float32) * 2 - 1).astype(np.float32)
    g = rng.standard_normal((x.shape[0], lay.n_output_dims), dtype=np.float32)
    if name == "d":
        g[D_COPIES] = g[D_COPIES.start]                 # the copies carry one upstream row, so their sum is 64 x one copy's
    for a in (x, table, g):
        a.setflags(write=False)
    return cfg, x, table, g
