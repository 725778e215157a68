"""The trainable tetrahedral SDF grid on the GPU (csrc/mesh_tets.hip, gaussianip_amd/utils/isosurface.py): marching tetrahedra forward
and backward, tet_sdf_diff, the helper and TetrahedraSDFGrid, and the loop they close with the mesh rasterizer.

Parity is against tests/golden/isosurface.npz, the float64 values of the reference's threestudio/models/isosurface.py and tet_sdf_diff
on the three cases of tests/isosurface_inputs.py (the reference's 32-grid, tests/golden/tets_32.npz):
  faces and the vertex count   exactly.
  vertices                     max |kernel - float64| <= 4 x the reference's own float32 error + 1.2e-7, and bit for bit the float32
                               restatement of the formula on the CPU (tests/isosurface_reference.py) from the same float32 positions.
  gradients, tet_sdf_diff      the error normalised by the quantity's maximum, at most 4 x the reference's own float32 error
                               (normalised the same way) + 1e-6.  Every entry of every quantity is compared.
With GIP_ISOSURFACE_PARITY_OUT=<file> the figures are written there as JSON (profiles/isosurface_parity.json is such a run)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import field_inputs
import isosurface_inputs as inputs
import isosurface_reference as reference

pytestmark = pytest.mark.gpu
FACTOR, FLOOR, VERTEX_FLOOR = 4.0, 1e-6, 1.2e-7
_figures = {}


@pytest.fixture(scope="module", autouse=True)
def _write_figures():
    yield
    out = os.environ.get("GIP_ISOSURFACE_PARITY_OUT")
    if out and _figures:
        with open(out, "w") as f:
            f.write(json.dumps(_figures, indent=1, sort_keys=True) + "\n")


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _counts():
    from gaussianip_amd import _lib
    return dict(_lib.call_counts)


def _launches(before):
    after = _counts()
    return {k: after[k] - before.get(k, 0) for k in after if after[k] != before.get(k, 0)}


def _rule(name, got, f64, ref_abs_err):
    """The gradients' rule of the module's docstring; ref_abs_err is the fixture's max |float32 - float64| of the reference."""
    got, f64 = np.asarray(got, np.float64), np.asarray(f64, np.float64)
    assert got.shape == f64.shape and np.isfinite(got).all(), name
    mx = np.abs(f64).max()
    assert mx > 0, name
    ref_err = float(ref_abs_err) / mx
    err = float(np.abs(got - f64).max() / mx)
    bar = FACTOR * ref_err + FLOOR
    print("%s: kernel %.3e reference %.3e bar %.3e (maximum %.3e)" % (name, err, ref_err, bar, mx))
    _figures[name] = dict(kernel_err=err, reference_err=ref_err, bar=bar, maximum=float(mx))
    assert err <= bar, (name, err, ref_err, bar)


@functools.lru_cache(maxsize=None)
def _helper():
    from gaussianip_amd.utils.isosurface import MarchingTetrahedraHelper
    return MarchingTetrahedraHelper(inputs.RESOLUTION, inputs.TETS).cuda()


def _edges_of(faces):
    """(unique undirected edges [E, 2], how many faces have each) of a face list on the GPU."""
    f = faces.long()
    e = torch.cat((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]))
    return torch.unique(torch.sort(e, dim=1)[0], dim=0, return_counts=True)


def _incident(grid, sdf):
    """[Nv] bool: the grid vertices with a crossing edge."""
    occ = sdf.reshape(-1) > 0
    a, b = grid.edges[:, 0], grid.edges[:, 1]
    cross = occ[a] != occ[b]
    hit = torch.zeros(grid.num_vertices, dtype=torch.bool, device=sdf.device)
    hit[a[cross]] = True
    hit[b[cross]] = True
    return hit


def _run(name):
    """One forward + backward of the helper and of tet_sdf_diff on a case: a dictionary of tensors."""
    from gaussianip_amd.utils.isosurface import tet_sdf_diff
    helper = _helper()
    gold = inputs.load_golden()
    sdf_np, def_np = inputs.case(name)
    sdf = _cu(sdf_np).requires_grad_(True)
    out = {}
    if def_np is not None:
        leaf = _cu(def_np).requires_grad_(True)
        mesh = helper(sdf, leaf)
    else:                                   # no deformation: the gradient to the grid's own positions, through the function itself
        from gaussianip_amd.utils.isosurface import marching_tetrahedra
        mesh = helper(sdf)
        assert mesh.extras["grid_deformation"] is None and mesh.extras["grid_vertices"] is helper.grid_vertices
        leaf = helper.grid_vertices.clone().requires_grad_(True)
        v2, f2 = marching_tetrahedra(helper.grid, sdf, leaf)
        assert torch.equal(v2, mesh.v_pos) and torch.equal(f2, mesh.t_pos_idx)
        mesh.v_pos = v2
    out["v_pos"], out["faces"], out["positions"] = mesh.v_pos.detach(), mesh.t_pos_idx, mesh.extras["grid_vertices"].detach()
    if out["v_pos"].shape[0] == gold[name + "_w"].shape[0]:
        w = _cu(gold[name + "_w"])
        out["g_sdf"], out["g_def" if def_np is not None else "g_pos"] = torch.autograd.grad((w * mesh.v_pos).sum(), (sdf, leaf))
    s2 = _cu(sdf_np).requires_grad_(True)
    val = tet_sdf_diff(s2, helper.grid)
    out["tsd"], (out["g_tsd"],) = val.detach(), torch.autograd.grad(val, s2)
    out["mesh"] = mesh
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("name", inputs.CASES)
def test_parity_with_the_reference(name):
    gold = inputs.load_golden()
    helper = _helper()
    assert np.array_equal(_np(helper.all_edges), gold["all_edges"]) and helper.all_edges.dtype == torch.int64
    before = _counts()
    got = _run(name)
    assert _launches(before) == {"gip_tet_mark": 1 if name == "noise" else 2, "gip_tet_emit": 1 if name == "noise" else 2,
                                 "gip_tet_backward": 1, "gip_tet_workspace_size": 1, "gip_tet_sdf_diff": 1, "gip_tet_sdf_diff_backward": 1}
    # faces and the vertex count: exactly
    assert got["faces"].dtype == torch.int32 and got["v_pos"].dtype == torch.float32
    assert got["v_pos"].shape == gold[name + "_v_pos"].shape
    assert np.array_equal(_np(got["faces"]), gold[name + "_faces"])
    mesh = got["mesh"]
    assert mesh.extras["tet_edges"] is helper.all_edges and mesh.extras["grid_level"].shape == (5034, 1)
    # vertices: the bar against float64, and the bits of the float32 restatement on the CPU from the same positions
    ref = gold[name + "_v_pos"]
    err = float(np.abs(_np(got["v_pos"]).astype(np.float64) - ref).max())
    bar = FACTOR * float(gold[name + "_err_v_pos"]) + VERTEX_FLOOR
    sdf_np, _ = inputs.case(name)
    _, tets = inputs.grid()
    cpu32, cpu_faces = reference.marching_tetrahedra(got["positions"].cpu(), torch.from_numpy(sdf_np), torch.from_numpy(tets))
    bit_equal = bool(torch.equal(cpu32, got["v_pos"].cpu()))
    differing = int((cpu32 != got["v_pos"].cpu()).sum())
    print("%s_v_pos: kernel %.3e reference %.3e bar %.3e; bit-equal to the float32 restatement: %s (%d entries differ)" % (
        name, err, float(gold[name + "_err_v_pos"]), bar, bit_equal, differing))
    _figures[name + "_v_pos"] = dict(kernel_abs_err=err, reference_abs_err=float(gold[name + "_err_v_pos"]), bar=bar,
                                     bit_equal_to_float32_restatement=bit_equal, entries_differing=differing)
    assert err <= bar, (name, err, bar)
    assert np.array_equal(cpu_faces.numpy(), gold[name + "_faces"])
    assert bit_equal, "%d entries differ from the float32 restatement" % differing
    # gradients and the regulariser
    for q in inputs.QUANTITIES[name][1:]:
        _rule("%s_%s" % (name, q), _np(got[q]).reshape(gold["%s_%s" % (name, q)].shape), gold["%s_%s" % (name, q)],
              gold["%s_err_%s" % (name, q)])
    # a grid vertex without a crossing edge: exact zeros
    quiet = ~_incident(helper.grid, _cu(sdf_np))
    assert quiet.any() and not got["g_sdf"][quiet].any()
    assert not got["g_def" if "g_def" in got else "g_pos"][quiet].any() and got["g_sdf"].any()


# ---------------------------------------------------------------------------------------------------------------- 2. reproducible
def test_bit_reproducible():
    first, second = _run("noise"), _run("noise")
    for q in ("v_pos", "faces", "g_sdf", "g_def", "tsd", "g_tsd"):
        assert torch.equal(first[q], second[q]), q
    side = torch.cuda.Stream()                      # nor do the bits depend on the stream
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = _run("noise")
    torch.cuda.current_stream().wait_stream(side)
    for q in ("v_pos", "faces", "g_sdf", "g_def", "tsd", "g_tsd"):
        assert torch.equal(first[q], third[q]), q


# ---------------------------------------------------------------------------------------------------------------- 3. edge cases
def test_one_sign_gives_an_empty_mesh():
    from gaussianip_amd.utils.isosurface import marching_tetrahedra, tet_sdf_diff
    grid = _helper().grid
    for value in (1.0, -1.0, 0.0):                  # all occupied, none occupied, and zeros, which are not occupied
        sdf = torch.full((grid.num_vertices, 1), value, device="cuda").requires_grad_(True)
        pos = grid.vertices.clone().requires_grad_(True)
        before = _counts()
        v, f = marching_tetrahedra(grid, sdf, pos)
        assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == torch.float32 and f.dtype == torch.int32
        (v.sum() + 0.0).backward()
        assert _launches(before) == {"gip_tet_mark": 1}               # nothing after the mark and the scan
        assert sdf.grad.shape == sdf.shape and not sdf.grad.any() and pos.grad.shape == pos.shape and not pos.grad.any()
        # no edge whose signs differ: the regulariser is a zero on the graph (a departure: the reference gives NaN)
        s = sdf.detach().clone().requires_grad_(True)
        val = tet_sdf_diff(s, grid)
        val.backward()
        assert float(val.detach()) == 0.0 and not s.grad.any()


def test_one_negative_vertex_gives_a_closed_fan():
    from gaussianip_amd.utils.isosurface import marching_tetrahedra
    grid = _helper().grid
    centre = int(((grid.vertices - 0.5) ** 2).sum(1).argmin())
    sdf = torch.ones(grid.num_vertices, device="cuda")
    sdf[centre] = -1.0
    sdf.requires_grad_(True)
    v, f = marching_tetrahedra(grid, sdf)                               # sdf as [Nv], positions = the grid's
    tets = grid.indices.long()
    case = ((sdf.detach()[tets] > 0).long() * torch.tensor([1, 2, 4, 8], device="cuda")).sum(1)
    count = torch.tensor(reference.NUM_TRIANGLES, device="cuda")[case]
    incident = (tets == centre).any(1)
    assert int(incident.sum()) >= 4 and not count[~incident].any()
    assert f.shape[0] == int(count[incident].sum()) == int(incident.sum())
    assert v.shape[0] == int((grid.edges == centre).any(1).sum())       # a vertex on every edge of the centre
    edges, faces_per_edge = _edges_of(f)
    assert torch.equal(faces_per_edge, torch.full_like(faces_per_edge, 2))
    assert torch.equal(torch.unique(f.long()), torch.arange(v.shape[0], device="cuda"))
    mid = 0.5 * (grid.vertices[grid.edges[:, 0]] + grid.vertices[grid.edges[:, 1]])[(grid.edges == centre).any(1)]
    assert torch.equal(v, mid)                                          # -1 against +1: the midpoints, exactly
    v.sum().backward()
    assert sdf.grad.shape == (grid.num_vertices,) and sdf.grad.any()


def test_positions_without_gradient_and_arguments():
    from gaussianip_amd.utils.isosurface import TetGrid, marching_tetrahedra, tet_sdf_diff
    helper = _helper()
    grid = helper.grid
    sdf_np, def_np = inputs.case("noise")
    sdf = _cu(sdf_np).requires_grad_(True)
    pos = (helper.grid_vertices + helper.normalize_grid_deformation(_cu(def_np))).detach()
    v, f = marching_tetrahedra(grid, sdf, pos)                          # positions need no gradient: that output is skipped
    assert not f.requires_grad and v.requires_grad
    w = _cu(inputs.load_golden()["noise_w"])
    (w * v).sum().backward()
    assert torch.equal(sdf.grad, _run("noise")["g_sdf"])
    # a non-contiguous sdf is the same sdf
    wide = torch.zeros((grid.num_vertices, 3), device="cuda")
    wide[:, 1] = sdf.detach()[:, 0]
    v2, f2 = marching_tetrahedra(grid, wide[:, 1], pos)
    assert torch.equal(v2, v) and torch.equal(f2, f)
    for bad in (sdf.double(), sdf.cpu(), sdf[:-1], sdf.reshape(1, -1)):
        with pytest.raises(ValueError, match="float32 GPU tensor"):
            marching_tetrahedra(grid, bad)
        with pytest.raises(ValueError, match="float32 GPU tensor"):
            tet_sdf_diff(bad, grid)
    with pytest.raises(ValueError, match="TetGrid"):
        marching_tetrahedra(grid.edges, sdf)
    with pytest.raises(ValueError, match="same device"):
        marching_tetrahedra(grid.to("cpu"), sdf)
    for bad in (pos.double(), pos.cpu(), pos[:-1]):
        with pytest.raises(ValueError, match="positions"):
            marching_tetrahedra(grid, sdf, bad)
    assert grid.to("cuda") is grid and torch.equal(grid.to("cpu").to("cuda").vert_edge_list, grid.vert_edge_list)
    # non-finite distances give non-finite vertices and nothing else
    s = sdf.detach().clone()
    s[::7] = float("nan")
    s[3::11] = float("inf")
    v3, f3 = marching_tetrahedra(grid, s, pos)
    assert int(f3.max()) < v3.shape[0] and int(f3.min()) >= 0 and not torch.isfinite(v3).all()
    assert not torch.isfinite(tet_sdf_diff(s, grid))


def test_kuhn_sphere_is_watertight_and_wound_outward():
    from gaussianip_amd.utils.isosurface import TetGrid, marching_tetrahedra
    grid = TetGrid.kuhn(8, device="cuda")
    assert grid.num_vertices == 729 and grid.num_tets == 6 * 512
    sdf = (grid.vertices - 0.5).norm(dim=1) - 0.3                       # strictly inside the grid; inside is negative
    v, f = marching_tetrahedra(grid, sdf)
    edges, faces_per_edge = _edges_of(f)
    assert f.shape[0] > 100 and torch.equal(faces_per_edge, torch.full_like(faces_per_edge, 2))
    assert v.shape[0] - edges.shape[0] + f.shape[0] == 2                # a sphere
    p = v.double()[f.long()]
    volume = float((torch.cross(p[:, 0], p[:, 1], dim=1) * p[:, 2]).sum() / 6.0)
    ball = 4.0 / 3.0 * np.pi * 0.3 ** 3
    print("signed volume %.5f of a ball of %.5f" % (volume, ball))
    assert 0.8 * ball < volume < ball                                   # inscribed-ish: positive, a little under the ball's
    ref_v, ref_f = reference.marching_tetrahedra(grid.vertices, sdf, grid.indices)
    assert torch.equal(ref_f.int(), f) and float((ref_v - v).abs().max()) <= 4 * 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- 4. the module
def test_tetrahedra_sdf_grid():
    """initialize_shape("sphere") and isosurface() in a non-unit bbox against the restatement in float64 from the module's own float32
    sdf.  The bar: a vertex in grid coordinates (at most 1) carries the roundings of two divisions, two products and a sum, the
    scaling to the bbox a subtraction, a division, a product and a sum on values of at most 1.5: 16 units of 2^-24 x 1.5 covers them."""
    from gaussianip_amd.utils.isosurface import TetrahedraSDFGrid
    geom = TetrahedraSDFGrid(isosurface_resolution=8, shape_init="sphere", shape_init_params=0.6, radius=1.5).cuda()
    assert sorted(n for n, _ in geom.named_parameters()) == ["deformation", "sdf"] and "isosurface_bbox" in dict(geom.named_buffers())
    assert geom.sdf.shape == (729, 1) and geom.deformation.shape == (729, 3) and not geom.sdf.any()
    assert torch.equal(geom.isosurface_bbox, torch.tensor([[-1.5] * 3, [1.5] * 3], device="cuda"))
    geom.initialize_shape()
    helper = geom.isosurface_helper
    points = reference.scale_tensor(helper.grid_vertices, (0, 1), geom.isosurface_bbox)
    assert float((geom.sdf.detach() - (points.norm(dim=1, keepdim=True) - 0.6)).abs().max()) <= 2.0 ** -22      # distances of at most 2.6
    mesh = geom.isosurface()
    ref_v, ref_f = reference.marching_tetrahedra(helper.grid_vertices.double(), geom.sdf.detach().double(), helper.grid.indices)
    ref_v = reference.scale_tensor(ref_v, (0, 1), geom.isosurface_bbox.double())
    assert torch.equal(mesh.t_pos_idx, ref_f.int()) and mesh.v_pos.requires_grad
    assert float((mesh.v_pos.detach().double() - ref_v).abs().max()) <= 16 * 2.0 ** -24 * 1.5
    radius = mesh.v_pos.detach().norm(dim=1)
    assert 0.5 < float(radius.min()) and float(radius.max()) < 0.61      # chords of a sphere of radius 0.6 on cells of 0.375
    # gradients arrive on both parameters, through the mesh's own terms
    (mesh.laplacian() + mesh.normal_consistency() + mesh.v_pos.sum()).backward()
    assert geom.sdf.grad.any() and geom.deformation.grad.any() and torch.isfinite(geom.sdf.grad).all()
    assert geom.isosurface() is not mesh                                # not fixed: a new mesh per call
    # an ellipsoid; no deformable grid; what is out of scope
    ell = TetrahedraSDFGrid(isosurface_resolution=8, isosurface_deformable_grid=False, shape_init="ellipsoid",
                            shape_init_params=(0.7, 0.5, 0.3)).cuda()
    ell.initialize_shape()
    assert ell.deformation is None and [n for n, _ in ell.named_parameters()] == ["sdf"]
    extent = ell.isosurface().v_pos.detach().abs().amax(0)
    assert torch.allclose(extent, torch.tensor([0.7, 0.5, 0.3], device="cuda"), atol=0.05)
    with pytest.raises(NotImplementedError, match="clean_mesh"):
        TetrahedraSDFGrid(isosurface_resolution=4, isosurface_remove_outliers=True)
    with pytest.raises(NotImplementedError, match="trimesh"):
        TetrahedraSDFGrid(isosurface_resolution=4, shape_init="mesh:a.obj", shape_init_params=1.0).initialize_shape()
    with pytest.raises(ValueError):
        TetrahedraSDFGrid(isosurface_resolution=4, shape_init="cube").initialize_shape()
    # fix_geometry: buffers, and the first mesh is kept
    fixed = TetrahedraSDFGrid(isosurface_resolution=8, shape_init="sphere", shape_init_params=0.6, fix_geometry=True).cuda()
    fixed.initialize_shape()
    assert list(fixed.parameters()) == [] and {"sdf", "deformation", "isosurface_bbox"} <= set(dict(fixed.named_buffers()))
    before = _counts()
    first = fixed.isosurface()
    fixed.sdf.add_(0.05)
    assert fixed.isosurface() is first and _launches(before) == {"gip_tet_mark": 1, "gip_tet_emit": 1}
    assert first.t_pos_idx.shape[0] > 0 and not first.requires_grad


def test_from_the_gaussians():
    from gaussianip_amd.scene import GaussianModel
    from gaussianip_amd.utils.isosurface import TetrahedraSDFGrid
    cl, R, nb = field_inputs.case("b")
    gm = GaussianModel(0)
    gm._xyz, gm._opacity = _cu(cl["xyz"]), _cu(cl["opacity"])
    gm._scaling, gm._rotation = _cu(cl["scaling"]), _cu(cl["rotation"])
    P = cl["xyz"].shape[0]
    gm._features_dc, gm._features_rest = torch.zeros((P, 1, 3), device="cuda"), torch.zeros((P, 0, 3), device="cuda")
    gm.extract_fields(resolution=R, num_blocks=nb)                      # sets center and scale
    lo, hi = gm.center - 1.0 / gm.scale, gm.center + 1.0 / gm.scale
    probe = TetrahedraSDFGrid(isosurface_resolution=12).isosurface_helper.grid_vertices.cuda()
    points = (probe * (hi - lo) + lo).contiguous()
    density = gm.sample_fields(points, resolution=R, num_blocks=nb)["density"]
    thresh = 0.5 * float(density.max())
    assert thresh > 0
    before = _counts()
    geom = gm.to_tetrahedra_sdf_grid(resolution=12, density_thresh=thresh, field_resolution=R, num_blocks=nb)
    assert _launches(before).get("gip_field_sample") == 1
    assert isinstance(geom, TetrahedraSDFGrid) and geom.sdf.is_cuda and geom.sdf.shape == (13 ** 3, 1) and not geom.deformation.any()
    assert torch.equal(geom.isosurface_bbox, torch.stack((lo, hi)))
    assert torch.equal(geom.sdf.detach(), (thresh - density).clamp(-1, 1).reshape(-1, 1))
    assert float(geom.sdf.min()) < 0 < float(geom.sdf.max())            # inside is negative
    mesh = geom.isosurface()
    assert mesh.t_pos_idx.shape[0] > 0 and mesh.v_pos.requires_grad
    assert bool((mesh.v_pos.detach() >= lo).all()) and bool((mesh.v_pos.detach() <= hi).all())
    with pytest.raises(TypeError):
        gm.to_tetrahedra_sdf_grid(resolution=12, colors=None)


# ---------------------------------------------------------------------------------------------------------------- 5. the loop closes
STEPS = 30


def test_the_loop_closes():
    """A sphere of radius 0.3 fitted to the antialiased silhouette of a sphere of radius 0.4 at 64 x 64, through
    DiffMeshRasterizerContext: MSE + a small tet_sdf_diff + the Laplacian loss.  The gradient reaches sdf only at grid vertices with a
    crossing edge; after STEPS Adam steps the loss is below where it started and the face count has changed, which a mesh of fixed
    connectivity cannot do."""
    from gaussianip_amd.utils.isosurface import TetrahedraSDFGrid, tet_sdf_diff
    from gaussianip_amd.utils.rasterize import DiffMeshRasterizerContext
    ctx = DiffMeshRasterizerContext()                                   # nothing below draws a random number
    mvp = torch.diag(torch.tensor([1.0, 1.0, 0.5, 1.0])).cuda()[None]  # the bbox [-1, 1]^3 seen along z, without perspective

    def silhouette(mesh):
        pos = ctx.vertex_transform(mesh.v_pos, mvp).contiguous()
        rast, _ = ctx.rasterize(pos, mesh.t_pos_idx, (64, 64))
        return ctx.antialias((rast[..., 3:] > 0).float(), rast, pos, mesh.t_pos_idx)

    with torch.no_grad():
        goal = TetrahedraSDFGrid(isosurface_resolution=24, shape_init="sphere", shape_init_params=0.4, fix_geometry=True).cuda()
        goal.initialize_shape()
        target = silhouette(goal.isosurface())
    geom = TetrahedraSDFGrid(isosurface_resolution=24, shape_init="sphere", shape_init_params=0.3).cuda()
    geom.initialize_shape()
    grid = geom.isosurface_helper.grid
    optimizer = torch.optim.Adam(geom.parameters(), lr=0.01)
    losses, face_counts = [], []
    for step in range(STEPS + 1):
        optimizer.zero_grad()
        mesh = geom.isosurface()
        loss = ((silhouette(mesh) - target) ** 2).mean() + 0.01 * tet_sdf_diff(geom.sdf, grid) + 0.1 * mesh.laplacian()
        losses.append(float(loss))
        face_counts.append(int(mesh.t_pos_idx.shape[0]))
        if step == STEPS:
            break
        loss.backward()
        if step == 0:
            g = geom.sdf.grad.reshape(-1)
            touched = _incident(grid, geom.sdf.detach())
            assert torch.isfinite(g).all() and g.any() and not g[~touched].any()
            assert torch.isfinite(geom.deformation.grad).all() and geom.deformation.grad.any()
            assert not geom.deformation.grad[~touched].any()
        optimizer.step()
    print("loss %.5f -> %.5f, faces %d -> %d" % (losses[0], losses[-1], face_counts[0], face_counts[-1]))
    print("losses", " ".join("%.5f" % x for x in losses))
    print("faces", face_counts)
    _figures["loop"] = dict(steps=STEPS, loss_first=losses[0], loss_last=losses[-1], faces_first=face_counts[0], faces_last=face_counts[-1])
    assert losses[-1] < losses[0] and face_counts[-1] != face_counts[0]
