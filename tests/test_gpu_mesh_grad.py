"""Gradients to vertex positions and the antialias pass on the GPU (csrc/mesh_grad.hip, DiffMeshRasterizerContext and the keywords
position_gradients / antialias of render_mesh in gaussianip_amd/utils/rasterize.py).

Everything is compared with tests/mesh_grad_reference.py, the kernel file's header restated in numpy, under the rule of
tests/test_gpu_mesh_render.py: errors normalised by the output's maximum, at most 4 times the float32 error of the restatement
against itself in float64 plus a floor of 2e-6; the restatement's error is computed here and printed.  The restatement's own
gradients are checked against central differences in tests/test_mesh_grad_cpu.py.  The decisions of the antialias pass are exact
integers in the kernel and in the restatement alike, so no pixel pair is left out of any comparison.

With GIP_MESH_GRAD_PARITY_OUT=<file> the figures are written there as JSON (profiles/mesh_grad_parity.json is such a run)."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import mesh_grad_inputs as grad_inputs
import mesh_grad_reference as gref
import mesh_render_inputs as inputs
import mesh_render_reference as ref
import sample_inputs
import scenes

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 4.0, 2e-6
H, W = inputs.H, inputs.W
_figures = {}


@pytest.fixture(scope="module", autouse=True)
def _write_figures():
    yield
    out = os.environ.get("GIP_MESH_GRAD_PARITY_OUT")
    if out and _figures:
        with open(out, "w") as f:
            f.write(json.dumps(_figures, indent=1, sort_keys=True) + "\n")


def _ctx():
    from gaussianip_amd.utils.rasterize import DiffMeshRasterizerContext
    return DiffMeshRasterizerContext()


def _plain():
    from gaussianip_amd.utils.rasterize import MeshRasterizerContext
    return MeshRasterizerContext()


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _rule(name, got, f64, f32):
    """The rule of the module's docstring; returns the bar (relative to the output's maximum)."""
    got, f64 = np.asarray(got, np.float64), np.asarray(f64, np.float64)
    assert np.isfinite(got).all(), name
    mx = np.abs(f64).max()
    assert mx > 0, name
    ref_err = float(np.abs(np.asarray(f32, np.float64) - f64).max() / mx)
    err = float(np.abs(got - f64).max() / mx)
    bar = FACTOR * ref_err + FLOOR
    print("%s: kernel %.3e reference %.3e bar %.3e" % (name, err, ref_err, bar))
    _figures[name] = dict(kernel_err=err, reference_err=ref_err, bar=bar)
    assert err <= bar, (name, err, ref_err, bar)
    return bar


def _ids(rast):
    return _np(rast[..., 3]).astype(np.int64) - 1


def _counts():
    from gaussianip_amd import _lib
    return dict(_lib.call_counts)


def _launches(before):
    after = _counts()
    return {k: after[k] - before.get(k, 0) for k in after if after[k] != before.get(k, 0)}


class _Cam:
    def __init__(self, proj, h=H, w=W):
        self.full_proj_transform, self.image_height, self.image_width = _cu(proj), h, w


MIRROR = np.diag([-1, 1, 1, 1]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- 1. rast -> pos
@functools.lru_cache(maxsize=None)
def _grid():
    """The jittered grid under its strongly perspective views (w spans 1 : 20), and one triangle behind it that no pixel shows."""
    pos, tri = inputs.grid_views()
    assert pos[..., 3].max() / pos[..., 3].min() > 15
    hidden = inputs._clip([[-0.5, -0.5], [0.5, -0.4], [0.0, 0.6]], np.full(3, 0.95), np.array([2.0, 3.0, 5.0]))
    pos = np.concatenate((pos, np.stack((hidden, hidden))), 1)
    tri = np.concatenate((tri, [[63, 64, 65]])).astype(np.int32)
    ids = ref.rasterize(pos, tri, H, W)["tri"]
    assert not (ids == 96).any() and (ids >= 0).all()
    return pos, tri, ids


def test_rasterize_backward():
    pos, tri, ids = _grid()
    g = np.random.default_rng(70).normal(size=(2, H, W, 4)).astype(np.float32)
    p = _cu(pos).requires_grad_(True)
    before = _counts()
    rast, db = _ctx().rasterize(p, _cu(tri), (H, W))
    assert db is None and rast.requires_grad
    (rast * _cu(g)).sum().backward()
    assert _launches(before) == {"gip_mesh_rasterize": 1, "gip_mesh_rasterize_backward": 1}
    plain, _ = _plain().rasterize(_cu(pos), _cu(tri), (H, W))
    assert torch.equal(rast.detach(), plain) and np.array_equal(_ids(rast), ids)
    want = {dt: gref.rasterize_grad(pos, tri, H, W, ids, g, dt) for dt in (np.float64, np.float32)}
    got = _np(p.grad)
    assert got.shape == pos.shape
    for c, name in enumerate("xyzw"):                                  # every component under its own maximum
        _rule("rasterize_backward_" + name, got[..., c], want[np.float64][..., c], want[np.float32][..., c])
    _rule("rasterize_backward", got, want[np.float64], want[np.float32])
    for b in range(2):
        used = np.zeros(pos.shape[1], bool)
        used[tri[np.unique(ids[b])].ravel()] = True
        assert not used[63:].any() and not got[b][~used].any() and np.abs(got[b][used]).min(1).max() > 0
    # one view as [V, 4], and a pos without a gradient
    one, _ = _ctx().rasterize_one(_cu(pos[1]).requires_grad_(True), _cu(tri), (H, W))
    assert one.requires_grad and torch.equal(one.detach(), plain[1])
    assert not _ctx().rasterize(_cu(pos), _cu(tri), (H, W))[0].requires_grad


# ---------------------------------------------------------------------------------------------------------------- 2. values -> rast
def test_interpolate_gradient_to_rast():
    pos, tri, ids = _grid()
    ctx = _ctx()
    rng = np.random.default_rng(71)
    rast = ctx.rasterize(_cu(pos), _cu(tri), (H, W))[0].requires_grad_(True)
    attr = rng.normal(size=(pos.shape[1], 5)).astype(np.float32)
    own_idx = rng.integers(0, 40, (len(tri), 3)).astype(np.int32)
    own_attr = rng.normal(size=(2, 40, 5)).astype(np.float32)           # one set of rows per view, indexed by its own tensor
    g = rng.normal(size=(2, H, W, 5)).astype(np.float32)
    for name, a, idx in (("shared", attr, tri), ("own", own_attr, own_idx)):
        rast.grad = None
        a_gpu = _cu(a).requires_grad_(True)
        before = _counts()
        out, _ = ctx.interpolate(a_gpu, rast, _cu(idx))
        (out * _cu(g)).sum().backward()
        assert _launches(before) == {"gip_mesh_interpolate": 1, "gip_mesh_interpolate_backward": 1, "gip_mesh_interpolate_backward_rast": 1}
        got = _np(rast.grad)
        _rule("interpolate_rast_%s_index" % name, got[..., :2], gref.interpolate_grad_rast(a, idx, ids, g, np.float64)[..., :2],
              gref.interpolate_grad_rast(a, idx, ids, g, np.float32)[..., :2])
        assert not got[..., 2:].any() and a_gpu.grad is not None
    # the default context detaches rast, as it always did
    rast.grad = None
    out, _ = _plain().interpolate(_cu(attr).requires_grad_(True), rast, _cu(tri))
    out.sum().backward()
    assert rast.grad is None
    # through to the positions: rasterize -> interpolate -> loss
    p = _cu(pos).requires_grad_(True)
    r, _ = ctx.rasterize(p, _cu(tri), (H, W))
    out, _ = ctx.interpolate(_cu(attr), r, _cu(tri))
    (out * _cu(g)).sum().backward()
    want = {dt: gref.rasterize_grad(pos, tri, H, W, ids, gref.interpolate_grad_rast(attr, tri, ids, g, dt), dt) for dt in (np.float64, np.float32)}
    _rule("interpolate_to_pos", _np(p.grad), want[np.float64], want[np.float32])


@functools.lru_cache(maxsize=None)
def _shade_case():
    """The grid seen by two exact cameras (inputs.EXACT_PROJ and its mirror image), a random 5 x 5 texture and OBJ texture coordinates
    that reach outside [0, 1]."""
    rng = np.random.default_rng(72)
    clip, tri = inputs.grid_mesh(1000)
    world = inputs.world_of(clip)
    projs = (inputs.EXACT_PROJ, MIRROR @ inputs.EXACT_PROJ)
    homogeneous = np.concatenate((world, np.ones((len(world), 1), np.float32)), 1)
    pos = np.stack([homogeneous @ m for m in projs])
    assert np.array_equal(pos[0], inputs.exact_clip(world))
    uv = rng.uniform(-0.5, 1.5, (len(tri), 3, 2)).astype(np.float32)
    flipped = np.stack((uv[..., 0], np.float32(1) - uv[..., 1]), -1)
    ids = ref.rasterize(pos, tri, H, W)["tri"]
    return dict(world=world, pos=pos, tri=tri, uv=uv, flipped=flipped, tex=rng.uniform(0, 1, (5, 5, 3)).astype(np.float32),
                bg=np.array([0.25, 0.5, 0.75], np.float32), ids=ids, projs=projs,
                b64=ref.barycentrics(pos, tri, H, W, ids, np.float64), b32=ref.barycentrics(pos, tri, H, W, ids, np.float32))


def test_render_mesh_gradient_to_vertices():
    from gaussianip_amd.utils.rasterize import render_mesh
    c = _shade_case()
    rng = np.random.default_rng(73)
    g = rng.normal(size=(2, H, W, 3)).astype(np.float32)
    gd = rng.normal(size=(2, H, W)).astype(np.float32)
    cams = [_Cam(m) for m in c["projs"]]
    world, tex = _cu(c["world"]).requires_grad_(True), _cu(c["tex"]).requires_grad_(True)
    before = _counts()
    out = render_mesh(cams, world, _cu(c["tri"]), _cu(c["uv"]), tex, bg_color=c["bg"], position_gradients=True)
    ((out["image"] * _cu(g).permute(0, 3, 1, 2)).sum() + (out["depth"][:, 0] * _cu(gd)).sum()).backward()
    assert _launches(before) == {"gip_mesh_rasterize": 1, "gip_mesh_shade": 1, "gip_mesh_shade_backward": 1,
                                 "gip_mesh_shade_backward_rast": 1, "gip_mesh_rasterize_backward": 1}
    with torch.no_grad():
        plain = render_mesh(cams, _cu(c["world"]), _cu(c["tri"]), _cu(c["uv"]), _cu(c["tex"]), bg_color=c["bg"])
    assert all(torch.equal(out[k].detach(), plain[k]) for k in plain) and np.array_equal(_ids(out["rast"]), c["ids"])
    want = {}
    for dt, key in ((np.float64, "b64"), (np.float32, "b32")):
        g_rast = gref.shade_grad_rast(c["tex"], c["flipped"], c["ids"], c[key][0], c[key][1], g, dt)
        g_rast[..., 2] = gd
        g_pos = gref.rasterize_grad(c["pos"], c["tri"], H, W, c["ids"], g_rast, dt)
        want[dt] = sum(g_pos[b] @ c["projs"][b].astype(dt).T for b in range(2))[:, :3]       # pos = (x, 1) @ proj
        if dt is np.float64:
            colour_only = g_rast.copy()
            colour_only[..., 2] = 0
            assert np.abs(gref.rasterize_grad(c["pos"], c["tri"], H, W, c["ids"], colour_only, dt)).max() > 0.01 * np.abs(g_pos).max()
    _rule("render_mesh_vertices", _np(world.grad), want[np.float64], want[np.float32])
    # the fused shade's gradient to rast on its own
    from gaussianip_amd.utils.rasterize import _Shade
    rast = out["rast"].detach().clone().requires_grad_(True)
    shaded = _Shade.apply(_cu(c["tex"]), _cu(c["uv"]), rast, _cu(c["bg"]), 1)
    (shaded[..., :3] * _cu(g)).sum().backward()
    w64, w32 = (gref.shade_grad_rast(c["tex"], c["flipped"], c["ids"], c[k][0], c[k][1], g, dt) for dt, k in ((np.float64, "b64"), (np.float32, "b32")))
    _rule("shade_rast", _np(rast.grad)[..., :2], w64[..., :2], w32[..., :2])
    assert not _np(rast.grad)[..., 2:].any()


# ---------------------------------------------------------------------------------------------------------------- 3. antialias
@functools.lru_cache(maxsize=None)
def _silhouettes():
    pos, tri = grad_inputs.silhouette_views()
    assert pos[1, :, 3].max() / pos[1, :, 3].min() > 10                  # the second view: strong perspective
    out = ref.rasterize(pos, tri, H, W)
    topo = gref.edge_topology(tri)
    hits = gref.antialias_hits(pos, tri, topo, out["tri"], out["depth"], H, W)
    tags = grad_inputs.TAGS
    for b in range(2):
        mine = [h for h in hits if h["b"] == b]
        assert len(mine) > 150 and {h["axis"] for h in mine} == {0, 1} and {h["s"] for h in mine} == {-1, 1}
        assert any(h["face"] in tags["fold"] and h["edge"] == 2 for h in mine)                 # the fold blends
        assert any(h["face"] in tags["near"] and out["tri"][(b,) + h["other"]] in tags["far"] for h in mine)      # quad over quad
        assert any(out["tri"][(b,) + h["other"]] < 0 for h in mine)                            # a boundary over the background
        assert not any(h["face"] in tags["three"] and h["edge"] == 2 for h in mine)            # the three-face edge never blends
        assert not any((h["face"], h["edge"]) in ((0, 1), (1, 2), (2, 1), (3, 0)) for h in mine)      # nor a quad's diagonal
        assert set(np.unique(out["tri"][b])) >= {-1, 0, 1, 2, 3, 4, 5, 6}
    return pos, tri, out["tri"], out["depth"], topo, hits


@pytest.mark.parametrize("C", [1, 5])
def test_antialias(C):
    from gaussianip_amd.utils.rasterize import edge_topology
    pos, tri, ids, depth, topo, hits = _silhouettes()
    ctx = _ctx()
    rng = np.random.default_rng(80 + C)
    color_np = (rng.uniform(0.2, 1, (2, H, W, C)) * (ids >= 0)[..., None] + rng.uniform(0, 0.2, (2, H, W, C))).astype(np.float32)
    g = rng.normal(size=(2, H, W, C)).astype(np.float32)
    t = _cu(tri)
    rast, _ = _plain().rasterize(_cu(pos), t, (H, W))
    assert np.array_equal(_ids(rast), ids) and np.array_equal(_np(rast[..., 2]), depth)
    table = edge_topology(t, pos.shape[1])
    assert table.is_cuda and np.array_equal(_np(table), topo)
    color, p = _cu(color_np).requires_grad_(True), _cu(pos).requires_grad_(True)
    before = _counts()
    out = ctx.antialias(color, rast, p, t)
    (out * _cu(g)).sum().backward()
    assert _launches(before) == {"gip_mesh_antialias": 1, "gip_mesh_antialias_backward": 1}
    _rule("antialias_C%d_out" % C, _np(out), gref.antialias(color_np, hits, pos, H, W, np.float64), gref.antialias(color_np, hits, pos, H, W, np.float32))
    w64, w32 = (gref.antialias_grad(color_np, hits, pos, g, H, W, dt) for dt in (np.float64, np.float32))
    _rule("antialias_C%d_g_color" % C, _np(color.grad), w64[0], w32[0])
    _rule("antialias_C%d_g_pos" % C, _np(p.grad), w64[1], w32[1])
    assert not _np(p.grad)[..., 2].any()
    on_an_edge = np.zeros(pos.shape[:2], bool)
    for h in hits:
        on_an_edge[h["b"], [h["iP"], h["iQ"]]] = True
    assert not _np(p.grad)[~on_an_edge].any()                           # nothing but a blending edge's two vertices moves
    # bit-identical on a second run, with the table passed in and from the context's cache alike
    with torch.no_grad():
        assert torch.equal(ctx.antialias(color, rast, p, t, topology=table), out) and torch.equal(ctx.antialias(color, rast, p, t), out)
    # a pixel whose four neighbours share its id keeps its colour bit for bit, and something else changed
    padded = np.pad(ids, ((0, 0), (1, 1), (1, 1)), mode="edge")
    same = ((padded[:, 1:-1, :-2] == ids) & (padded[:, 1:-1, 2:] == ids) & (padded[:, :-2, 1:-1] == ids) & (padded[:, 2:, 1:-1] == ids))
    assert np.array_equal(_np(out)[same], color_np[same]) and same.sum() > H * W
    changed = (_np(out) != color_np).any(-1)
    assert changed.sum() > 200 and not (changed & same).any()
    # the cache follows the tensor: edited in place, it is rebuilt
    mine = t.clone()
    first = ctx.antialias(color.detach(), rast, p.detach(), mine)
    assert torch.equal(first, out)
    mine[6:] = mine[6:].flip(0)                                          # the same faces in another order: rast no longer matches
    assert torch.equal(ctx._topology.get(mine, pos.shape[1]), edge_topology(mine, pos.shape[1]))


def test_row_sums_of_a_rectangle():
    """tests/test_mesh_grad_cpu.py's rectangle through the kernels: the row sums of the antialiased mask are the width, exactly (every t
    is a multiple of 1 / 256), and their gradient in the right-hand vertices' x is 0.5 W / w per row.  The gradient's bar: t's
    derivative, its scaling to clip space and the sum over 12 atomic adds are a dozen float32 roundings: 32 units of 2^-24."""
    h, w_img, w = 12, 16, 2.0
    x_lo, x_hi, y_lo, y_hi = 2 * 256 + 37, 12 * 256 + 201, 1 * 256 + 90, 10 * 256 + 150
    pos, tri = grad_inputs.rectangle(x_lo, x_hi, y_lo, y_hi, w, h, w_img)
    ctx = _ctx()
    p = _cu(pos).requires_grad_(True)
    rast, _ = ctx.rasterize(p, _cu(tri), (h, w_img))
    mask = (rast[..., 3:] > 0).float()
    out = ctx.antialias(mask, rast, p, _cu(tri))
    rows = out[0, 3:9, :, 0].double().sum(1)
    assert torch.equal(rows, torch.full_like(rows, (x_hi - x_lo) / 256)), rows
    rows.sum().backward()
    got, want = _np(p.grad)[0], 6 * 0.5 * w_img / w
    print("row-sum gradient: right %.9g left %.9g, expected +-%.9g" % (got[[1, 2], 0].sum(), got[[0, 3], 0].sum(), want))
    assert abs(got[[1, 2], 0].sum() - want) <= 32 * 2.0 ** -24 * want and abs(got[[0, 3], 0].sum() + want) <= 32 * 2.0 ** -24 * want


# ---------------------------------------------------------------------------------------------------------------- 4. why it exists
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


def test_a_mask_loss_moves_the_sphere_only_when_antialiased():
    """The sphere of tests/test_gpu_mesh_render.py (radius about 15 pixels at 96 x 96) against the mask of itself moved by about 1.5
    pixels along the camera's right axis.  Without the antialias pass the L2 mask loss has an exactly zero gradient in the vertices;
    with it the summed gradient points away from the target along that axis, so a descent step moves towards it, and its component
    along the camera's up axis is the smaller one.  The cosine between the descent direction and the shift is printed, without a bar."""
    from gaussianip_amd.scene import Camera
    from gaussianip_amd.utils.rasterize import render_mesh
    cl, rgb = sample_inputs.sphere_cloud()
    v, f, _, uv, texture = _model(cl, rgb).extract_textured_mesh(density_thresh=sample_inputs.SPHERE_THRESHOLD, resolution=32, num_blocks=4)
    size, dist, fovy = 96, 3.0, math.radians(20.0)
    c2w = scenes.orbit_c2w(10.0, 20.0, dist)
    rot = c2w[:3, :3].clone()
    c2w[:3, 3] -= rot @ torch.diag(torch.tensor([1.0, -1.0, -1.0])) @ rot.t() @ torch.tensor(sample_inputs.SPHERE_MU, dtype=torch.float32)
    cam = Camera(c2w=c2w.cuda(), FoVy=fovy, height=size, width=size)
    right, up = rot[:, 0].cuda(), rot[:, 1].cuda()
    shift = 1.5 * (2 * dist * math.tan(fovy / 2) / size) * right          # 1.5 pixels at the sphere's distance
    with torch.no_grad():
        target = render_mesh(cam, v + shift, f, uv, texture, antialias=True)["alpha"]
        start = render_mesh(cam, v, f, uv, texture, antialias=True)["alpha"]
    xs = torch.arange(size, device="cuda", dtype=torch.float32)
    centroid = lambda a: torch.stack(((a[0] * xs[None, :]).sum(), (a[0] * xs[:, None]).sum())) / a.sum()  # noqa: E731
    moved = _np(centroid(target) - centroid(start))
    print("the target's centroid is (%.3f, %.3f) pixels from the start's" % (moved[0], moved[1]))
    assert 1.2 < abs(moved[0]) < 1.8 and abs(moved[1]) < 0.2 and 0 <= float(target.min()) <= float(target.max()) <= 1
    blended = int(((target > 0) & (target < 1)).sum())
    print("%d pixels of the target's outline are blended" % blended)      # few: near the limb the faces are slivers, and a pair
    assert blended > 0                                                    # blends only across an edge of the near pixel's own face
    grads = {}
    for aa in (False, True):
        verts = v.clone().requires_grad_(True)
        out = render_mesh(cam, verts, f, uv, texture, position_gradients=True, antialias=aa)
        ((out["alpha"] - target) ** 2).sum().backward()
        grads[aa] = verts.grad
    assert grads[False] is not None and not grads[False].any()            # exactly zero: coverage is piecewise constant
    total = grads[True].sum(0)
    gx, gy = float(total @ right), float(total @ up)
    cosine = float(-total @ shift / (total.norm() * shift.norm()))
    print("summed gradient along right %.4e, along up %.4e; cosine between -gradient and the shift %.4f" % (gx, gy, cosine))
    _figures["sphere_mask_loss"] = dict(gradient_along_right=gx, gradient_along_up=gy, cosine=cosine, centroid_shift_px=moved.tolist())
    assert grads[True].any() and gx < 0 and abs(gy) < abs(gx)


# ---------------------------------------------------------------------------------------------------------------- 5. interface
def test_defaults_still_raise_and_argument_errors():
    from gaussianip_amd.utils.rasterize import edge_topology, render_mesh
    pos, tri, ids = _grid()
    ctx, plain = _ctx(), _plain()
    p, t = _cu(pos), _cu(tri)
    rast, _ = plain.rasterize(p, t, (H, W))
    with pytest.raises(NotImplementedError, match="antialias"):
        plain.antialias(rast, rast, p, t)
    with pytest.raises(NotImplementedError, match="pos"):
        plain.rasterize(p.clone().requires_grad_(True), t, (H, W))
    world = _cu(inputs.world_of(pos[0]))
    uv, tex = torch.zeros((len(tri), 3, 2), device="cuda"), torch.zeros((8, 8, 3), device="cuda")
    with pytest.raises(NotImplementedError, match="vertices"):
        render_mesh(_Cam(inputs.EXACT_PROJ), world.clone().requires_grad_(True), t, uv, tex)
    with pytest.raises(NotImplementedError, match="vertices"):
        render_mesh(_Cam(inputs.EXACT_PROJ), world.clone().requires_grad_(True), t, uv, tex, antialias=True)
    for c in (ctx, plain):
        with pytest.raises(NotImplementedError, match="rast_db"):
            c.interpolate(torch.zeros((pos.shape[1], 3), device="cuda"), rast, t, rast_db=rast)
        with pytest.raises(NotImplementedError, match="filter_mode"):
            c.texture(torch.zeros((1, 4, 4, 3), device="cuda"), torch.zeros((2, 4, 4, 2), device="cuda"), filter_mode="linear-mipmap-linear")
    color = torch.zeros((2, H, W, 3), device="cuda")
    table = edge_topology(t, pos.shape[1])
    for args in ((color.cpu(), rast, p, t), (color, rast.cpu(), p, t), (color, rast, p.cpu(), t), (color, rast, p, t.cpu()),
                 (color.double(), rast, p, t), (color, rast, p, t.long()), (color[:1], rast, p, t), (color[:, :-1], rast, p, t),
                 (color[..., :0], rast, p, t), (color, rast[..., :3], p, t), (color, rast, p[..., :3], t), (color, rast, p[:1], t)):
        with pytest.raises(ValueError):
            ctx.antialias(*args)
    for bad in (table.cpu(), table.long(), table[:-1], table.float()):
        with pytest.raises(ValueError, match="topology"):
            ctx.antialias(color, rast, p, t, topology=bad)
    for bad_tri, n in ((t.long(), 10), (t[:, :2], 10), (t, 0)):
        with pytest.raises(ValueError):
            edge_topology(bad_tri, n)
    for bad_pos, bad_tri in ((p.cpu(), t), (p, t.cpu()), (p.double(), t), (p[..., :3], t)):
        with pytest.raises(ValueError):
            ctx.rasterize(bad_pos.clone().requires_grad_(True), bad_tri, (H, W))
    # no faces: nothing to blend, nothing launched
    none = torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    before = _counts()
    assert torch.equal(ctx.antialias(color, torch.zeros_like(rast), p, none), color) and _launches(before) == {}
