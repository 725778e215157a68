"""Surface extraction on the GPU (csrc/field.hip marching tetrahedra, gaussianip_amd.utils.mesh.extract_surface) on analytic fields,
and GaussianModel.extract_mesh end to end.

Topology is checked exactly: in a closed surface every undirected edge is used by two faces, once in each direction.  The volume of
the sphere (r = 0.6 on [-1, 1]^3, R = 32) must be within 5 % of 4/3 pi r^3: the longest Kuhn edge is sqrt(3) h with h = 2 / 31, the
chord sagitta and the linear interpolation of a quadratic each cost at most 3 h^2 / (8 r) = 0.4 % of the radius, under 3 % of the
volume together."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _grid(R):
    g = torch.linspace(-1, 1, R, dtype=torch.float64)
    return torch.meshgrid(g, g, g, indexing="ij")


def _surface(f, thr):
    from gaussianip_amd import _lib
    from gaussianip_amd.utils.mesh import extract_surface
    before = _lib.call_counts.get("gip_surface_count", 0)
    v, fc = extract_surface(f.float().cuda(), thr)
    assert _lib.call_counts.get("gip_surface_count", 0) == before + 1
    assert v.dtype == torch.float32 and fc.dtype == torch.int32 and v.shape[1:] == (3,) and fc.shape[1:] == (3,)
    return v.cpu().numpy().astype(np.float64), fc.cpu().numpy().astype(np.int64)


def _edges(v, f):
    """(edges used twice, once per direction; edges used once; everything else) over the undirected edges, and the edge count."""
    assert f.size == 0 or (f.min() >= 0 and f.max() < len(v))
    assert not ((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 2] == f[:, 0])).any()
    d = np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]))
    code = d[:, 0] * (len(v) + 1) + d[:, 1]
    assert len(np.unique(code)) == len(code), "a directed edge is used by two faces"
    back = d[:, 1] * (len(v) + 1) + d[:, 0]
    paired = np.isin(code, back)
    return int(paired.sum()) // 2, int((~paired).sum()), int(paired.sum()) // 2 + int((~paired).sum())


def _closed_euler(v, f):
    twice, once, E = _edges(v, f)
    assert once == 0 and twice == E
    assert len(np.unique(f)) == len(v)          # every vertex is used
    return len(v) - E + len(f)


def _volume(v, f, R):
    w = v / (R - 1.0) * 2 - 1
    return float(np.einsum("ij,ij->i", w[f[:, 0]], np.cross(w[f[:, 1]], w[f[:, 2]])).sum() / 6)


def test_plane_vertices_lie_on_the_plane():
    R, a, b, thr = 20, np.array([0.3, -0.5, 0.8]), 0.1, 0.05
    x, y, z = _grid(R)
    v, f = _surface(a[0] * x + a[1] * y + a[2] * z + b, thr)
    assert len(v) > 100 and len(f) > 100
    p = v / (R - 1.0) * 2 - 1
    assert np.abs(p @ a + b - thr).max() <= 1e-5
    n = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
    assert (n @ a < 0).all()                    # normals toward decreasing values
    assert _edges(v, f)[1] > 0                  # the plane leaves the grid: an open boundary


@pytest.mark.parametrize("R", [32, 17])
def test_sphere_is_closed_and_oriented(R):
    x, y, z = _grid(R)
    r = 0.6
    v, f = _surface(r * r - (x * x + y * y + z * z), 0.0)
    assert _closed_euler(v, f) == 2
    vol = _volume(v, f, R)
    print("R %d: volume %.5f of %.5f" % (R, vol, 4 / 3 * math.pi * r ** 3))
    assert vol > 0
    if R == 32:
        assert abs(vol - 4 / 3 * math.pi * r ** 3) <= 0.05 * 4 / 3 * math.pi * r ** 3


def test_torus_has_genus_one():
    x, y, z = _grid(32)
    v, f = _surface(0.25 ** 2 - ((torch.sqrt(x * x + y * y) - 0.55) ** 2 + z * z), 0.0)
    assert _closed_euler(v, f) == 0


def test_two_spheres():
    x, y, z = _grid(32)
    one = 0.3 ** 2 - ((x - 0.45) ** 2 + y * y + z * z)
    two = 0.3 ** 2 - ((x + 0.45) ** 2 + y * y + z * z)
    v, f = _surface(torch.maximum(one, two), 0.0)
    assert _closed_euler(v, f) == 4


def test_sphere_cut_by_the_grid_boundary_stays_open():
    R = 32
    x, y, z = _grid(R)
    v, f = _surface(0.5 ** 2 - ((x - 0.8) ** 2 + y * y + z * z), 0.0)
    twice, once, E = _edges(v, f)
    assert once > 0 and twice > 0 and once + twice == E
    d = np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]))
    code, back = d[:, 0] * (len(v) + 1) + d[:, 1], d[:, 1] * (len(v) + 1) + d[:, 0]
    open_ends = v[d[~np.isin(code, back)].reshape(-1)]
    assert np.abs(open_ends[:, 0] - (R - 1)).max() <= 1e-6       # every boundary edge lies in the grid face x = +1


def test_values_equal_to_the_threshold():
    R = 17
    i = torch.arange(R, dtype=torch.float64)
    a, b, c = torch.meshgrid(i, i, i, indexing="ij")
    f = 4 - torch.maximum(torch.maximum((a - 8).abs(), (b - 8).abs()), (c - 8).abs())       # integers; the shell at distance 4 is == 0
    v, fc = _surface(f, 0.0)
    assert len(v) > 0 and np.isfinite(v).all() and v.min() >= 0 and v.max() <= R - 1
    assert fc.min() >= 0 and fc.max() < len(v)
    d = np.concatenate((fc[:, [0, 1]], fc[:, [1, 2]], fc[:, [2, 0]]))
    code, back = d[:, 0] * (len(v) + 1) + d[:, 1], d[:, 1] * (len(v) + 1) + d[:, 0]
    assert len(np.unique(code)) == len(code) and np.isin(code, back).all()      # still closed, index for index


def test_threshold_above_the_maximum_is_empty():
    x, y, z = _grid(16)
    v, f = _surface(0.6 ** 2 - (x * x + y * y + z * z), 1.0)
    assert v.shape == (0, 3) and f.shape == (0, 3)


def test_two_runs_are_identical():
    from gaussianip_amd.utils.mesh import extract_surface
    x, y, z = _grid(32)
    f = (0.25 ** 2 - ((torch.sqrt(x * x + y * y) - 0.55) ** 2 + z * z)).float().cuda()
    v1, f1 = extract_surface(f, 0.0)
    v2, f2 = extract_surface(f, 0.0)
    assert torch.equal(v1, v2) and torch.equal(f1, f2)


def test_argument_errors():
    from gaussianip_amd.utils.mesh import extract_surface
    with pytest.raises(ValueError):
        extract_surface(torch.zeros(8, 8, 8), 0.0)                      # not on the GPU
    with pytest.raises(ValueError):
        extract_surface(torch.zeros(8, 8, 4, device="cuda"), 0.0)


def test_extract_mesh_end_to_end(tmp_path):
    """2000 Gaussians on a Fibonacci sphere of radius 0.5, isotropic sigma 0.025, opacity 0.9: the density on the sphere is about
    0.9 * (2000 / (4 pi 0.25)) * 2 pi sigma^2 = 2.2, so density 1 is a closed shell (an outer and an inner surface)."""
    from gaussianip_amd.scene import GaussianModel
    from gaussianip_amd.utils.mesh import read_obj
    P = 2000
    k = np.arange(P) + 0.5
    phi, theta = np.arccos(1 - 2 * k / P), math.pi * (1 + 5 ** 0.5) * k
    pts = 0.5 * np.stack((np.sin(phi) * np.cos(theta), np.sin(phi) * np.sin(theta), np.cos(phi)), 1)
    gm = GaussianModel(0)
    gm._xyz = torch.from_numpy(pts.astype(np.float32)).cuda()
    gm._opacity = torch.full((P, 1), math.log(0.9 / 0.1), device="cuda")
    gm._scaling = torch.full((P, 3), math.log(0.025), device="cuda")
    gm._rotation = torch.zeros(P, 4, device="cuda")
    gm._rotation[:, 0] = 1
    path = tmp_path / "out" / "mesh.obj"
    v, f = gm.extract_mesh(path=str(path), resolution=64)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and v.is_cuda and len(v) > 1000
    vn, fn = v.cpu().numpy(), f.cpu().numpy()
    euler = _closed_euler(vn.astype(np.float64), fn.astype(np.int64))
    assert euler == 4                           # two spheres: the shell's outer and inner surface
    lo, hi = pts.min(0), pts.max(0)
    grow = 0.1 * (hi - lo)
    assert (vn >= lo - grow).all() and (vn <= hi + grow).all()
    rv, rf = read_obj(str(path))
    assert np.array_equal(rv, vn) and np.array_equal(rf, fn)
