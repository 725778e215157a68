"""The chart atlas on the GPU (csrc/mesh_uv.hip, gaussianip_amd/utils/uv_atlas.py, GaussianModel.bake_chart_texture /
extract_textured_mesh(atlas="charts")).

The unwrapper is pinned by tests/uv_atlas_reference.py, an independent numpy restatement whose float32 arithmetic is the kernels'
operation for operation: the integer outputs and v_tex are compared exactly.  The tangents are pinned by tests/golden/uv_tangents.npz
(the reference's Mesh._compute_vertex_tangent and autograd in float64) under the rule of the other reference fixtures: the error
normalised by the quantity's maximum, at most 4 times the reference's own float32 error plus a floor of 2e-6.  The texel points are held
to the mesh rasteriser's interpolation bar against tests/mesh_render_reference.py.  GIP_UV_ATLAS_PARITY_OUT names a JSON file that
receives the figures."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_geometry_inputs as inputs  # noqa: E402
import mesh_render_reference as raster_reference  # noqa: E402
import sample_inputs  # noqa: E402
import scenes  # noqa: E402
import uv_atlas_reference as reference  # noqa: E402

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 4.0, 2e-6
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "uv_tangents.npz")
T_UNWRAP = 256
_figures = {}


@pytest.fixture(scope="module", autouse=True)
def _write_figures():
    yield
    out = os.environ.get("GIP_UV_ATLAS_PARITY_OUT")
    if out and _figures:
        with open(out, "w") as f:
            json.dump(_figures, f, indent=1, sort_keys=True)


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _rule(name, got, f64, ref_err_abs):
    mx = float(np.abs(f64).max())
    ref_err = float(ref_err_abs) / mx
    err = float(np.abs(got.astype(np.float64) - f64).max() / mx)
    bar = FACTOR * ref_err + FLOOR
    print("%s: kernel %.3e reference %.3e bar %.3e (maximum %.3e)" % (name, err, ref_err, bar, mx))
    _figures[name] = dict(kernel_err=err, reference_err=ref_err, bar=bar, maximum=mx)
    assert err <= bar, (name, err, ref_err, bar)


def _unwrap(name, rounds, T=T_UNWRAP):
    from gaussianip_amd.utils.uv_atlas import unwrap_charts
    v, f, _, _ = inputs.mesh(name)
    return unwrap_charts(_cu(v), _cu(f), T, smooth_rounds=rounds), v, f


# ---------------------------------------------------------------------------------------------------------------- 1. the atlas
@pytest.mark.parametrize("name,rounds", [("a", 0), ("a", 4), ("b", 0), ("b", 4)])
def test_atlas_equals_the_restatement(name, rounds):
    atlas, v, f = _unwrap(name, rounds)
    want = reference.unwrap_mesh(name, T_UNWRAP, rounds)
    assert np.array_equal(_np(atlas.face_nbr), want["face_nbr"])
    assert np.array_equal(_np(atlas.face_chart), want["face_chart"]) and atlas.face_chart.dtype == torch.int32
    assert np.array_equal(_np(atlas.chart_class), want["chart_class"])
    assert atlas.num_charts == want["chart_class"].shape[0]
    assert np.array_equal(atlas.chart_box, want["chart_box"]) and atlas.chart_box.dtype == np.float32
    assert np.float32(atlas.scale) == want["scale"]
    assert np.array_equal(atlas.chart_rect, want["chart_rect"])
    assert np.array_equal(_np(atlas.t_tex_idx), want["t_tex_idx"]) and np.array_equal(_np(atlas.vmapping), want["vmapping"])
    got = _np(atlas.v_tex)
    diff = float(np.abs(got.astype(np.float64) - want["v_tex"].astype(np.float64)).max())
    print("%s rounds %d: %d charts, Vt %d, scale %.4f, max |v_tex - restatement| %.3e" % (
        name, rounds, atlas.num_charts, got.shape[0], atlas.scale, diff))
    _figures["v_tex_%s_%d" % (name, rounds)] = dict(max_abs_diff=diff, charts=atlas.num_charts, texture_vertices=int(got.shape[0]))
    assert np.array_equal(got.view(np.uint32), want["v_tex"].view(np.uint32))
    again, _, _ = _unwrap(name, rounds)
    for key in ("v_tex", "t_tex_idx", "vmapping", "face_chart", "chart_class"):
        assert torch.equal(getattr(atlas, key), getattr(again, key)), key
    assert np.array_equal(atlas.chart_rect, again.chart_rect)


@pytest.mark.parametrize("name,rounds", [("a", 0), ("a", 4), ("b", 0), ("b", 4)])
def test_atlas_properties(name, rounds):
    atlas, v, f = _unwrap(name, rounds)
    T, pad = atlas.texture_size, atlas.pad
    vt, tt, fc = _np(atlas.v_tex).astype(np.float64), _np(atlas.t_tex_idx).astype(np.int64), _np(atlas.face_chart).astype(np.int64)
    cls = _np(atlas.chart_class).astype(np.int64)[fc]
    assert vt.min() >= 0 and vt.max() <= 1
    xy = np.stack((vt[:, 0] * T - 0.5, (1 - vt[:, 1]) * T - 0.5), 1)                   # texel-index coordinates, exact in float64
    # orientation and kept area of every non-degenerate face
    p = v.astype(np.float64)[f.astype(np.int64)]
    n32 = reference.face_normals(v, f)
    d32 = n32[:, 0] * n32[:, 0] + n32[:, 1] * n32[:, 1] + n32[:, 2] * n32[:, 2]
    live = d32 > np.float32(1e-20)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    along = n[np.arange(len(n)), cls >> 1] * np.where(cls & 1, -1.0, 1.0)
    assert (along[live] >= 0.25 * np.linalg.norm(n[live], axis=1) * (1 - 1e-6)).all()
    q = xy[tt]
    area2 = (q[:, 1, 0] - q[:, 0, 0]) * (q[:, 2, 1] - q[:, 0, 1]) - (q[:, 1, 1] - q[:, 0, 1]) * (q[:, 2, 0] - q[:, 0, 0])
    assert (area2[live] > 0).all()
    # neighbours in one chart share the texture vertices of their common edge
    nbr = _np(atlas.face_nbr)
    shared = 0
    for i, k in zip(*np.nonzero(nbr >= 0)):
        g = int(nbr[i, k])
        if fc[g] != fc[i]:
            continue
        a, b = int(f[i, k]), int(f[i, (k + 1) % 3])
        ta, tb = int(tt[i, k]), int(tt[i, (k + 1) % 3])
        other = {int(f[g, j]): int(tt[g, j]) for j in range(3)}
        assert other[a] == ta and other[b] == tb
        shared += 1
    assert shared > len(f)
    # a texture vertex is its position vertex projected, scaled and placed in its chart's rectangle
    vm = _np(atlas.vmapping).astype(np.int64)
    chart_of = np.zeros(len(vm), np.int64)
    chart_of[tt.reshape(-1)] = np.repeat(fc, 3)
    u, w = reference.project(v[vm].astype(np.float64), _np(atlas.chart_class).astype(np.int64)[chart_of])
    box, rect = atlas.chart_box.astype(np.float64), atlas.chart_rect
    want_x = rect[chart_of, 0] + pad + (u - box[chart_of, 0]) * atlas.scale
    want_y = rect[chart_of, 1] + pad + (w - box[chart_of, 1]) * atlas.scale
    err = max(np.abs(xy[:, 0] - want_x).max(), np.abs(xy[:, 1] - want_y).max())
    print("%s rounds %d: texture vertices against the float64 placement: %.3e texels" % (name, rounds, err))
    assert err <= T * 2.0 ** -21                       # a handful of float32 roundings of numbers below T
    # every texture vertex at least pad texels inside its chart's rectangle
    assert (xy[:, 0] >= rect[chart_of, 0] + pad).all() and (xy[:, 0] <= rect[chart_of, 0] + rect[chart_of, 2] - 1 - pad).all()
    assert (xy[:, 1] >= rect[chart_of, 1] + pad).all() and (xy[:, 1] <= rect[chart_of, 1] + rect[chart_of, 3] - 1 - pad).all()


def test_degenerate_meshes():
    from gaussianip_amd import _lib
    from gaussianip_amd.utils.uv_atlas import unwrap_charts
    v = _cu(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.2]], np.float32))
    before = {k: _lib.call_counts.get(k, 0) for k in _lib.MESH_UV_SYMBOLS}
    empty = unwrap_charts(v, torch.zeros((0, 3), dtype=torch.int32, device="cuda"), 64)
    assert {k: _lib.call_counts.get(k, 0) for k in _lib.MESH_UV_SYMBOLS} == before       # F = 0 launches nothing
    assert tuple(empty.v_tex.shape) == (0, 2) and tuple(empty.t_tex_idx.shape) == (0, 3) and empty.num_charts == 0
    assert tuple(empty.chart_rect.shape) == (0, 4) and empty.vmapping.numel() == 0 and empty.face_chart.numel() == 0
    covered, points, face = empty.texel_points(v)
    assert not bool(covered.any()) and bool((face == -1).all()) and tuple(points.shape) == (64, 64, 3)
    one = unwrap_charts(v, _cu(np.array([[0, 1, 2]], np.int32)), 64)
    want = reference.unwrap(_np(v), np.array([[0, 1, 2]]), 64, 4)
    assert one.num_charts == 1 and one.chart_class.tolist() == [4] and one.t_tex_idx.tolist() == [[0, 1, 2]]
    assert np.array_equal(_np(one.v_tex).view(np.uint32), want["v_tex"].view(np.uint32)) and np.array_equal(one.chart_rect, want["chart_rect"])
    flipped = unwrap_charts(v, _cu(np.array([[0, 2, 1]], np.int32)), 64)
    assert flipped.chart_class.tolist() == [5]
    with pytest.raises(ValueError, match="indices"):
        unwrap_charts(v, _cu(np.array([[0, 1, 3]], np.int32)), 64)
    with pytest.raises(ValueError, match="min_cos"):
        unwrap_charts(v, _cu(np.array([[0, 1, 2]], np.int32)), 64, min_cos=0.7)
    sized = unwrap_charts(v, _cu(np.array([[0, 1, 2]], np.int32)), texels_per_unit=20.0)
    assert sized.texture_size == 32 and sized.chart_rect.tolist() == [[0, 0, 26, 26]] and sized.scale == 20.0


# ---------------------------------------------------------------------------------------------------------------- 2. tangents
def _tangent_inputs(name):
    from gaussianip_amd.utils.mesh_geometry import MeshTopology
    v, f, w, tags = inputs.mesh(name)
    atlas = reference.unwrap_mesh(name, T_UNWRAP, 4)
    with np.load(GOLDEN) as z:
        gold = {k[2:]: z[k] for k in z.files if k.startswith(name + "_")}
    topo = MeshTopology(_cu(f), v.shape[0])
    return v, f, w, tags, atlas, gold, topo


def _tangents(v, w, atlas, gold, topo):
    from gaussianip_amd.utils.uv_atlas import vertex_tangents
    x = _cu(v).requires_grad_(True)
    n = _cu(gold["nrm"]).requires_grad_(True)
    t = vertex_tangents(x, topo, _cu(atlas["v_tex"]), _cu(atlas["t_tex_idx"]), n)
    rows = _cu(gold["rows"].astype(np.int64))
    g_v, g_n = torch.autograd.grad((_cu(w)[rows] * t[rows]).sum(), (x, n))
    return t.detach(), g_v, g_n


@pytest.mark.parametrize("name", ["a", "b"])
def test_tangents_against_the_reference(name):
    v, f, w, tags, atlas, gold, topo = _tangent_inputs(name)
    t, g_v, g_n = _tangents(v, w, atlas, gold, topo)
    rows = gold["rows"].astype(np.int64)
    assert len(rows) + len(tags["unreferenced"]) == v.shape[0]
    _rule("%s_v_tng" % name, _np(t)[rows], gold["v_tng"], gold["err_v_tng"])
    _rule("%s_g_v" % name, _np(g_v)[rows], gold["g_v"], gold["err_g_v"])
    _rule("%s_g_nrm" % name, _np(g_n)[rows], gold["g_nrm"], gold["err_g_nrm"])
    lone = np.array(tags["unreferenced"], np.int64)
    assert len(lone) >= 2 and tags["isolated"] in lone
    assert np.array_equal(_np(t)[lone], np.tile(np.array([1, 0, 0], np.float32), (len(lone), 1)))
    assert not _np(g_v)[lone].any() and not _np(g_n)[lone].any()
    t2, g_v2, g_n2 = _tangents(v, w, atlas, gold, topo)
    assert torch.equal(t, t2) and torch.equal(g_v, g_v2) and torch.equal(g_n, g_n2)
    # unit length, perpendicular to the normal
    tn, nn = _np(t)[rows].astype(np.float64), gold["nrm"][rows].astype(np.float64)
    assert np.abs(np.linalg.norm(tn, axis=1) - 1).max() < 1e-5 and np.abs((tn * nn).sum(1)).max() < 1e-5


def test_uv_mesh():
    from gaussianip_amd.utils.mesh_geometry import Mesh
    from gaussianip_amd.utils.uv_atlas import UVMesh, unwrap_charts, vertex_tangents
    v, f, _, _ = inputs.mesh("a")
    mesh = UVMesh(_cu(v), _cu(f))
    atlas = unwrap_charts(_cu(v), _cu(f), 1024)
    assert torch.equal(mesh.v_tex, atlas.v_tex) and torch.equal(mesh.t_tex_idx, atlas.t_tex_idx)      # unwrapped on first use
    want = vertex_tangents(_cu(v), mesh.topology, atlas.v_tex, atlas.t_tex_idx, mesh.v_nrm)
    assert torch.equal(mesh.v_tng, want) and mesh.v_tng is mesh.v_tng and tuple(want.shape) == (v.shape[0], 3)
    small = mesh.unwrap_uv({}, {}, texture_size=256, smooth_rounds=0)
    assert small.texture_size == 256 and torch.equal(mesh.v_tex, unwrap_charts(_cu(v), _cu(f), 256, smooth_rounds=0).v_tex)
    with pytest.raises(ValueError, match="xatlas"):
        mesh.unwrap_uv({"max_iterations": 2})
    with pytest.raises(ValueError, match="xatlas"):
        mesh.unwrap_uv(xatlas_pack_options={"resolution": 512})
    assert float(mesh.laplacian()) > 0 and tuple(mesh.edges.shape)[1] == 2                             # inherited
    plain = Mesh(_cu(v), _cu(f))
    for member in ("v_tex", "t_tex_idx", "v_tng"):
        with pytest.raises(NotImplementedError):
            getattr(plain, member)
    with pytest.raises(NotImplementedError):
        plain.unwrap_uv()


# ---------------------------------------------------------------------------------------------------------------- 3. dilation
def _blobs():
    rng = np.random.default_rng(5)
    img = rng.uniform(0, 1, (37, 29, 3)).astype(np.float32)
    yy, xx = np.mgrid[:37, :29]
    mask = np.zeros((37, 29), bool)
    for cy, cx, r in ((6, 5, 3.2), (20, 18, 4.5), (33, 3, 2.0), (0, 28, 1.5), (30, 24, 0.5)):
        mask |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
    return img, mask


@pytest.mark.parametrize("rounds", [1, 3])
def test_dilation_equals_the_restatement(rounds):
    from gaussianip_amd.utils.uv_atlas import dilate_texture
    img, mask = _blobs()
    want, want_mask = reference.dilate(img, mask, rounds)
    got, got_mask = dilate_texture(_cu(img), _cu(mask), rounds)
    assert np.array_equal(_np(got_mask), want_mask) and want_mask.sum() > mask.sum() and not want_mask.all()
    assert np.array_equal(_np(got).view(np.uint32), want.view(np.uint32))
    again, _ = dilate_texture(_cu(img), _cu(mask), rounds)
    assert torch.equal(got, again)


def test_dilation_edge_cases():
    from gaussianip_amd.utils.uv_atlas import dilate_texture
    img, mask = _blobs()
    t, m = _cu(img), _cu(mask)
    same, same_mask = dilate_texture(t, m, 0)
    assert torch.equal(same, t) and torch.equal(same_mask, m)
    none, none_mask = dilate_texture(t, torch.zeros_like(m), 2)
    assert not bool(none.any()) and not bool(none_mask.any())
    full, full_mask = dilate_texture(t, torch.ones_like(m), 1)
    assert torch.equal(full, t) and bool(full_mask.all())
    far, far_mask = dilate_texture(t, m, 64)
    assert bool(far_mask.all()) and bool(torch.isfinite(far).all())
    with pytest.raises(ValueError):
        dilate_texture(t, m, -1)


# ---------------------------------------------------------------------------------------------------------------- 4. texel points
def test_texel_points():
    from gaussianip_amd.utils.uv_atlas import dilate_texture
    T = 128
    atlas, v, f = _unwrap("a", 4, T)
    want = reference.unwrap_mesh("a", T, 4)
    assert np.array_equal(_np(atlas.v_tex).view(np.uint32), want["v_tex"].view(np.uint32))
    covered, points, face = atlas.texel_points(_cu(v))
    vt = want["v_tex"]
    pos = np.concatenate((vt * np.float32(2) - np.float32(1), np.zeros_like(vt[:, :1]), np.ones_like(vt[:, :1])), 1)[None].astype(np.float32)
    tri = want["t_tex_idx"].astype(np.int64)
    ids = raster_reference.rasterize(pos, tri, T, T)["tri"]                       # the rasteriser's integer coverage rule
    assert np.array_equal(_np(face), ids[0][::-1]) and np.array_equal(_np(covered), ids[0][::-1] >= 0)
    occupancy = float((ids >= 0).mean())
    assert 0.2 < occupancy < 0.8
    attr = v[want["vmapping"]]
    res = {}
    for dt in (np.float64, np.float32):
        bu, bv, _ = raster_reference.barycentrics(pos, tri, T, T, ids, dt)
        res[dt] = raster_reference.interpolate(attr, tri, ids, bu, bv, dt)[0][::-1]
    _rule("texel_points", _np(points), res[np.float64], np.abs(res[np.float32].astype(np.float64) - res[np.float64]).max())
    assert not _np(points)[~_np(covered)].any()
    # a covered texel's point lies on its face: inside the face's bounding box, up to rounding
    tri_pos = v.astype(np.float64)[f.astype(np.int64)][_np(face)[_np(covered)]]
    pt = _np(points)[_np(covered)].astype(np.float64)
    assert (pt >= tri_pos.min(1) - 1e-5).all() and (pt <= tri_pos.max(1) + 1e-5).all()
    # after pad rounds of dilation every texel within pad of a covered one holds a colour
    colour = torch.where(covered.unsqueeze(2), points * 0.25 + 0.5, torch.zeros_like(points))
    out, filled = dilate_texture(colour, covered, atlas.pad)
    k = 2 * atlas.pad + 1
    near = torch.nn.functional.max_pool2d(covered[None, None].float(), k, 1, atlas.pad)[0, 0] > 0
    assert torch.equal(filled, near) and bool((out[filled].abs().sum(1) > 0).all()) and not bool(out[~filled].any())
    assert torch.equal(out[covered], colour[covered])
    _figures["occupancy_a_128"] = occupancy


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
def _model(cl, rgb):
    from gaussianip_amd.scene import GaussianModel
    from gaussianip_amd.utils.sh import C0
    gm = GaussianModel(0)
    gm._xyz, gm._opacity = _cu(cl["xyz"]), _cu(cl["opacity"])
    gm._scaling, gm._rotation = _cu(cl["scaling"]), _cu(cl["rotation"])
    P = cl["xyz"].shape[0]
    gm._features_dc = ((_cu(rgb) - 0.5) / C0).reshape(P, 1, 3).contiguous()
    return gm


def _camera(el, az, dist, target, fovy_deg, size):
    from gaussianip_amd.scene import Camera
    c2w = scenes.orbit_c2w(el, az, dist)
    rot = c2w[:3, :3].clone()
    c2w[:3, 3] -= rot @ torch.diag(torch.tensor([1.0, -1.0, -1.0])) @ rot.t() @ torch.tensor(target, dtype=torch.float32)
    return Camera(c2w=c2w.cuda(), FoVy=math.radians(fovy_deg), height=size, width=size)


def test_chart_textured_mesh_end_to_end(tmp_path):
    from gaussianip_amd.utils.mesh import read_obj_textured
    from gaussianip_amd.utils.rasterize import MipMeshRasterizerContext, MipStack, render_mesh
    cl = sample_inputs.blob_cloud()
    rgb = sample_inputs.colors(cl["xyz"].shape[0], 9)
    gm = _model(cl, rgb)
    kw = dict(density_thresh=1.0, resolution=32, num_blocks=4)
    obj = tmp_path / "out" / "charts.obj"
    v, f, n, uv, texture = gm.extract_textured_mesh(path=str(obj), atlas="charts", **kw)
    F, T = int(f.shape[0]), int(texture.shape[0])
    assert F > 100 and tuple(uv.shape) == (F, 3, 2) and tuple(texture.shape) == (T, T, 3) and T & (T - 1) == 0
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["charts.mtl", "charts.obj", "charts_kd.png"]
    rv, rf, rn, ruv, rtex, v_tex, t_tex_idx = read_obj_textured(str(obj), return_index=True)
    assert np.array_equal(rv, _np(v)) and np.array_equal(rf, _np(f)) and np.array_equal(rn, _np(n)) and np.array_equal(ruv, _np(uv))
    assert 0 < v_tex.shape[0] < 3 * F and tuple(t_tex_idx.shape) == (F, 3)
    print("%d faces, %d texture vertices (3 F = %d), texture %d" % (F, v_tex.shape[0], 3 * F, T))
    assert rtex.shape == tuple(texture.shape) and np.abs(rtex - _np(texture)).max() <= 0.5 / 255 + 1e-7
    assert float(texture.min()) >= 0 and float(texture.max()) <= 1 + 1e-6 and float(texture.max()) > 0.2
    # the per-face path is untouched by the keyword
    plain = gm.extract_textured_mesh(**kw)
    named = gm.extract_textured_mesh(atlas="faces", **kw)
    assert all(torch.equal(a, b) for a, b in zip(plain, named))
    assert torch.equal(plain[0], v) and torch.equal(plain[1], f)
    with pytest.raises(NotImplementedError, match="per-face atlas"):
        gm.extract_textured_mesh(atlas="charts", bake="views", cameras=[None], **kw)
    with pytest.raises(ValueError, match="atlas"):
        gm.extract_textured_mesh(atlas="xatlas", **kw)
    # the mip path takes the texture: the stack builds, and with the level clamped to 0 it is the bilinear render bit for bit
    size = 64
    target = [float(x) for x in _np(v).mean(0)]
    cam = _camera(15.0, 30.0, 3.0, target, 40.0, size)
    ctx = MipMeshRasterizerContext()
    stack = ctx.texture_construct_mip(texture)
    assert isinstance(stack, MipStack) and stack.L == int(math.log2(T))
    pos = torch.matmul(torch.cat((v, torch.ones_like(v[:, :1])), 1)[None], cam.full_proj_transform.to(v.device).float()[None]).contiguous()
    rast, rast_db = ctx.rasterize(pos, f, (size, size))
    internal = torch.stack((uv[..., 0], 1 - uv[..., 1]), -1).reshape(3 * F, 2).contiguous()      # the lookup's own convention: v down
    corner = torch.arange(3 * F, dtype=torch.int32, device="cuda").reshape(F, 3)
    st, st_da = ctx.interpolate(internal, rast, corner, rast_db, "all")
    bilinear = ctx.texture(texture, st, filter_mode="linear")
    clamped = ctx.texture(texture, st, uv_da=st_da, max_mip_level=0)
    assert torch.equal(clamped, bilinear)
    mipped = ctx.texture(texture, st, uv_da=st_da, mip=stack)
    hit = rast[0, :, :, 3] > 0
    assert int(hit.sum()) > 200 and bool(torch.isfinite(mipped).all())
    shaded = render_mesh(cam, v, f, uv, texture)
    assert torch.equal(shaded["alpha"][0] > 0, hit)
    assert float((shaded["image"].permute(1, 2, 0)[hit] - bilinear[0][hit]).abs().max()) <= 1e-5


def test_bake_chart_texture():
    from gaussianip_amd.utils.uv_atlas import unwrap_charts
    cl, rgb = sample_inputs.sphere_cloud()
    gm = _model(cl, rgb)
    kw = dict(resolution=32, num_blocks=4)
    v, f = gm.extract_mesh(density_thresh=sample_inputs.SPHERE_THRESHOLD, **kw)
    atlas = unwrap_charts(v, f, 128)
    baked = gm.bake_chart_texture(v, f, atlas, **kw)
    covered, filled, texture = baked["covered"], baked["filled"], baked["texture"]
    assert torch.equal(baked["uv"], atlas.uv) and int(covered.sum()) > 1000 and int(filled.sum()) > int(covered.sum())
    colour = np.array(sample_inputs.SPHERE_COLOR, np.float32)
    err = float(np.abs(_np(texture)[_np(filled)] - colour).max())                     # one colour everywhere, padding included
    print("sphere: %d charts, %d covered, %d filled texels, colour error %.3e" % (atlas.num_charts, int(covered.sum()), int(filled.sum()), err))
    _figures["sphere_chart_colour_err"] = err
    assert err <= 1e-5 and not bool(texture[~filled].any())
    with pytest.raises(ValueError, match="ChartAtlas"):
        gm.bake_chart_texture(v, f[:-1].contiguous(), atlas, **kw)
