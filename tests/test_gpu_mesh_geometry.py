"""The geometry terms of the mesh on the GPU (csrc/mesh_geom.hip, gaussianip_amd/utils/mesh_geometry.py): vertex normals, the uniform
Laplacian loss and the normal consistency, forward and backward.

Parity is against tests/golden/mesh_geometry.npz, the float64 values of the reference's threestudio/models/mesh.py on the two meshes of
tests/mesh_geometry_inputs.py, under the rule of tests/test_gpu_mesh_render.py / test_gpu_mesh_grad.py: the error normalised by the
quantity's maximum, at most 4 times the reference's own float32 error (`err` in the fixture, normalised the same way) plus a floor of
2e-6.  Every entry of every quantity is compared.

With GIP_MESH_GEOMETRY_PARITY_OUT=<file> the figures are written there as JSON (profiles/mesh_geometry_parity.json is such a run)."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import mesh_geometry_inputs as inputs
import sample_inputs
import scenes

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 4.0, 2e-6
_figures = {}


@pytest.fixture(scope="module", autouse=True)
def _write_figures():
    yield
    out = os.environ.get("GIP_MESH_GEOMETRY_PARITY_OUT")
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
    """The rule of the module's docstring; ref_abs_err is the fixture's max |float32 - float64| of the reference."""
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
def _case(name):
    from gaussianip_amd.utils.mesh_geometry import MeshTopology
    v, f, w, tags = inputs.mesh(name)
    return _cu(v), MeshTopology(_cu(f), v.shape[0]), _cu(w), tags


def _terms(v, topo, w):
    """(normals, laplacian, consistency, their three gradients) of one forward + backward of each term."""
    from gaussianip_amd.utils import mesh_geometry as mg
    out = []
    for fn in (lambda x: (w * mg.vertex_normals(x, topo)).sum(), lambda x: mg.laplacian_loss(x, topo), lambda x: mg.normal_consistency(x, topo)):
        x = v.clone().requires_grad_(True)
        val = fn(x)
        g, = torch.autograd.grad(val, x)
        out.append((val.detach(), g))
    with torch.no_grad():
        n = mg.vertex_normals(v, topo)
    return n, out[1][0], out[2][0], out[0][1], out[1][1], out[2][1]


# ---------------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("name", ["a", "b"])
def test_parity_with_the_reference(name):
    gold = inputs.load_golden()
    v, topo, w, tags = _case(name)
    assert topo.num_edges == gold[name + "_edges"].shape[0] and np.array_equal(_np(topo.edges), gold[name + "_edges"])
    before = _counts()
    got = dict(zip(inputs.QUANTITIES, _terms(v, topo, w)))
    assert _launches(before) == {"gip_mesh_vertex_normals": 3, "gip_mesh_vertex_normals_backward": 2, "gip_mesh_laplacian_loss": 1,
                                 "gip_mesh_laplacian_loss_backward": 1, "gip_mesh_normal_consistency": 1,
                                 "gip_mesh_normal_consistency_backward": 1, "gip_mesh_geometry_workspace_size": 2}
    assert got["lap"].shape == () and got["nc"].shape == () and got["v_nrm"].shape == tuple(v.shape)
    for q in inputs.QUANTITIES:
        _rule("%s_%s" % (name, q), _np(got[q]), gold["%s_%s" % (name, q)], gold["%s_err_%s" % (name, q)])
    if name == "b":          # the fan's apex, a row longer than a wave, agrees with the fixture on its own
        apex = tags["apex"]
        for q in ("v_nrm", "g_nrm", "g_lap", "g_nc"):
            ref = gold["b_" + q]
            bar = FACTOR * float(gold["b_err_" + q]) + FLOOR * np.abs(ref).max()
            assert np.abs(ref[apex]).max() > 0 and np.abs(_np(got[q])[apex] - ref[apex]).max() <= bar, q


# ---------------------------------------------------------------------------------------------------------------- 2. conventions
def test_cases_the_reference_defines_by_convention():
    from gaussianip_amd.utils import mesh_geometry as mg
    v, topo, w, tags = _case("a")
    n, lap, nc, g_nrm, g_lap, g_nc = _terms(v, topo, w)
    lone = list(tags["unreferenced"])
    assert tags["isolated"] in lone
    assert torch.equal(n[lone], torch.tensor([0.0, 0.0, 1.0], device="cuda").expand(len(lone), 3))
    for g in (g_nrm, g_lap, g_nc):
        assert not g[lone].any() and g.any()
    assert torch.equal(n.norm(dim=1) > 0.999, torch.ones(n.shape[0], dtype=torch.bool, device="cuda"))
    # the face with a repeated index: E counts its pair (a, a), and nothing else changes
    _, f, _, _ = inputs.mesh("a")
    without = mg.MeshTopology(_cu(np.delete(f, tags["repeated_face"], 0)), v.shape[0])
    assert without.num_edges == topo.num_edges - 1 and torch.equal(without.nbr_list, topo.nbr_list)
    n2, lap2, nc2, g_nrm2, g_lap2, g_nc2 = _terms(v, without, w)
    assert torch.equal(n2, n) and torch.equal(lap2, lap) and torch.equal(g_lap2, g_lap)      # its cross product is an exact zero
    # in the normals' backward its corners 0 and 1, both at vertex a, take -x and +x with x = (p_b - p_a) x g_face: they cancel in exact
    # arithmetic, and in float32 leave the rounding of two additions in a's running sum, each at most 2^-24 of a gradient-sized value
    ulp = 2.0 ** -24
    assert float((g_nrm2 - g_nrm).abs().max()) <= 16 * ulp * float(g_nrm.abs().max())
    moved = (g_nrm2 != g_nrm).any(1).nonzero().reshape(-1).tolist()
    assert set(moved) <= {tags["self_pair"][0]}
    E = topo.num_edges
    assert abs(float(nc) * E - float(nc2) * (E - 1)) <= 4 * ulp * float(nc) * E             # the same sum under another count
    assert float(nc2) > float(nc) and float((g_nc2 * (E - 1) - g_nc * E).abs().max()) <= 16 * ulp * float(g_nc.abs().max()) * E


# ---------------------------------------------------------------------------------------------------------------- 3. reproducible
def test_bit_reproducible():
    v, topo, w, _ = _case("b")
    first, second = _terms(v, topo, w), _terms(v, topo, w)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    # nor do the bits depend on what else the device is doing: the same terms on a second stream, next to the first
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = _terms(v, topo, w)
    torch.cuda.current_stream().wait_stream(side)
    for a, b in zip(first, third):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- 4. interface
def test_mesh_class():
    from gaussianip_amd.utils import mesh_geometry as mg
    v, topo, w, _ = _case("a")
    _, f, _, _ = inputs.mesh("a")
    n, lap, nc, _, g_lap, g_nc = _terms(v, topo, w)
    x = v.clone().requires_grad_(True)
    before = _counts()
    mesh = mg.Mesh(x, _cu(f).long(), note="kept")                     # int64 faces, as code written against the reference passes
    assert mesh.requires_grad and mesh.extras == {"note": "kept"} and mesh._topology is None
    assert torch.equal(mesh.v_nrm.detach(), n) and mesh.v_nrm is mesh.v_nrm and mesh.topology is mesh.topology
    assert torch.equal(mesh.edges, topo.edges) and mesh.edges.dtype == torch.int64
    assert mesh.v_nrm[mesh.edges].shape == (topo.num_edges, 2, 3)         # the reference's own indexing of normals by edges
    assert torch.equal(mesh.laplacian().detach(), lap)
    assert torch.equal(mesh.normal_consistency().detach(), nc)
    got, = torch.autograd.grad(mesh.normal_consistency(), x)
    assert torch.equal(got, g_nc)
    got, = torch.autograd.grad(mesh.laplacian(), x)
    assert torch.equal(got, g_lap)
    ran = _launches(before)
    for sym in ("gip_mesh_vertex_normals", "gip_mesh_vertex_normals_backward", "gip_mesh_laplacian_loss", "gip_mesh_laplacian_loss_backward",
                "gip_mesh_normal_consistency", "gip_mesh_normal_consistency_backward"):
        assert ran.get(sym, 0) >= 1, sym
    assert ran["gip_mesh_vertex_normals"] == 1                        # v_nrm is computed once and kept
    for attr in ("v_tng", "v_tex", "t_tex_idx"):
        with pytest.raises(NotImplementedError):
            getattr(mesh, attr)
    with pytest.raises(NotImplementedError, match="atlas"):
        mesh.unwrap_uv()
    with pytest.raises(NotImplementedError, match="clean_mesh"):
        mesh.remove_outlier(0.1)
    mesh.set_vertex_color(torch.ones_like(v))
    assert mesh.v_rgb.shape == v.shape


def test_arguments_and_empty_meshes():
    from gaussianip_amd.utils import mesh_geometry as mg
    v, topo, w, _ = _case("a")
    for fn in (mg.vertex_normals, mg.laplacian_loss, mg.normal_consistency):
        with pytest.raises(ValueError, match="float32 GPU tensor"):
            fn(v.double(), topo)
        with pytest.raises(ValueError, match="float32 GPU tensor"):
            fn(v.cpu(), topo)
        with pytest.raises(ValueError, match="float32 GPU tensor"):
            fn(v[:, :2], topo)
        with pytest.raises(ValueError, match="built for"):
            fn(v[:-1], topo)
        with pytest.raises(ValueError, match="MeshTopology"):
            fn(v, topo.faces)
        with pytest.raises(ValueError, match="same device"):
            fn(v, topo.to("cpu"))
    assert topo.to("cuda") is topo and torch.equal(topo.to("cpu").to("cuda").nbr_list, topo.nbr_list)
    # no faces: default normals, zero losses, zero gradients, and no launch
    none = mg.MeshTopology(torch.zeros((0, 3), dtype=torch.int32, device="cuda"), 5)
    x = v[:5].clone().requires_grad_(True)
    before = _counts()
    n = mg.vertex_normals(x, none)
    total = n.sum() + mg.laplacian_loss(x, none) + mg.normal_consistency(x, none)
    total.backward()
    assert _launches(before) == {}
    assert torch.equal(n.detach(), torch.tensor([0.0, 0.0, 1.0], device="cuda").expand(5, 3)) and float(total.detach()) == 5.0 and not x.grad.any()
    # a non-contiguous view of the vertices is the same mesh
    wide = torch.zeros((v.shape[0], 5), device="cuda")
    wide[:, 1:4] = v
    assert torch.equal(mg.laplacian_loss(wide[:, 1:4], topo), mg.laplacian_loss(v, topo))
    # double backward: PyTorch's default error and no further
    x = v.clone().requires_grad_(True)
    g, = torch.autograd.grad(mg.laplacian_loss(x, topo), x, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


# ---------------------------------------------------------------------------------------------------------------- 5. with the renderer
def _model(cl, colors):
    from gaussianip_amd.scene import GaussianModel
    from gaussianip_amd.utils.sh import C0
    gm = GaussianModel(0)
    gm._xyz, gm._opacity = _cu(cl["xyz"]), _cu(cl["opacity"])
    gm._scaling, gm._rotation = _cu(cl["scaling"]), _cu(cl["rotation"])
    P = cl["xyz"].shape[0]
    gm._features_dc = ((_cu(colors) - 0.5) / C0).reshape(P, 1, 3).contiguous()
    gm._features_rest = torch.zeros((P, 0, 3), device="cuda")
    return gm


def test_one_loss_with_the_renderer():
    """The sphere of tests/test_gpu_mesh_grad.py's mask-loss test at 96 x 96: coverage against the mask of the sphere moved by 1.5 pixels,
    through render_mesh(position_gradients=True, antialias=True), plus lambda times the Laplacian loss, as one loss.  Its gradient is
    finite and is the sum of the two terms' own gradients.  The bar: the Laplacian term is bit-reproducible, and its sum with the
    coverage gradient is one float32 addition per entry (2^-24 relative); the renderer's backward adds a vertex's per-pixel
    contributions with float atomics, so two runs of it differ by the reordering of float32 additions, at most a few hundred per
    vertex, each worth 2^-24 of the running sum: 256 x 2^-24 of the coverage gradient's maximum covers both."""
    from gaussianip_amd.scene import Camera
    from gaussianip_amd.utils import mesh_geometry as mg
    from gaussianip_amd.utils.rasterize import render_mesh
    cl, rgb = sample_inputs.sphere_cloud()
    v, f, _, uv, texture = _model(cl, rgb).extract_textured_mesh(density_thresh=sample_inputs.SPHERE_THRESHOLD, resolution=32, num_blocks=4)
    size, dist, fovy = 96, 3.0, math.radians(20.0)
    c2w = scenes.orbit_c2w(10.0, 20.0, dist)
    rot = c2w[:3, :3].clone()
    c2w[:3, 3] -= rot @ torch.diag(torch.tensor([1.0, -1.0, -1.0])) @ rot.t() @ torch.tensor(sample_inputs.SPHERE_MU, dtype=torch.float32)
    cam = Camera(c2w=c2w.cuda(), FoVy=fovy, height=size, width=size)
    shift = 1.5 * (2 * dist * math.tan(fovy / 2) / size) * rot[:, 0].cuda()
    with torch.no_grad():
        target = render_mesh(cam, v + shift, f, uv, texture, antialias=True)["alpha"]
    topo = mg.MeshTopology(f, v.shape[0])
    lam = 100.0

    def coverage(x):
        return ((render_mesh(cam, x, f, uv, texture, position_gradients=True, antialias=True)["alpha"] - target) ** 2).sum()

    def grad_of(fn):
        x = v.clone().requires_grad_(True)
        fn(x).backward()
        return x.grad

    before = _counts()
    both = grad_of(lambda x: coverage(x) + lam * mg.laplacian_loss(x, topo))
    ran = _launches(before)
    assert ran["gip_mesh_laplacian_loss_backward"] == 1 and ran["gip_mesh_antialias_backward"] == 1
    g_cov, g_lap = grad_of(coverage), grad_of(lambda x: lam * mg.laplacian_loss(x, topo))
    assert torch.isfinite(both).all() and g_cov.any() and g_lap.any()
    bar = 256 * 2.0 ** -24 * float(g_cov.abs().max())
    err = float((both - (g_cov + g_lap)).abs().max())
    print("one loss: |joint - (coverage + laplacian)| %.3e, bar %.3e; maxima %.3e and %.3e" % (err, bar, float(g_cov.abs().max()), float(g_lap.abs().max())))
    _figures["joint_loss"] = dict(err=err, bar=bar, coverage_max=float(g_cov.abs().max()), laplacian_max=float(g_lap.abs().max()))
    assert float(g_lap.abs().max()) > bar                 # the regulariser is visible at that bar
    assert err <= bar
