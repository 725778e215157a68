"""The mesh rasterizer on the GPU (csrc/mesh_raster.hip, gaussianip_amd/utils/rasterize.py, GaussianModel.render_textured_mesh).

Coverage, the winning triangle and its depth are compared bit for bit with tests/mesh_render_reference.py, the definition restated in
numpy.  Everything computed in floating point after that (barycentrics, interpolation, lookup, shade, gradients) follows the rule of
tests/test_gpu_field.py: errors normalised by the output's maximum, at most 4 times the float32 error of the restatement against
itself in float64 plus a floor of 2e-6; the restatement's error is computed here and printed.

With GIP_MESH_RENDER_PARITY_OUT=<file> the figures are written there as JSON (profiles/mesh_render_parity.json is such a run); with
GIP_MESH_RENDER_PROFILE_OUT=<the JSON of tools/bench_mesh_render.py> the alignment test adds its centroids and PSNR to that file
(profiles/mesh_render.json, key "alignment_test_128")."""
import functools
import json
import math
import os
from argparse import ArgumentParser

import numpy as np
import pytest
import torch

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
    out = os.environ.get("GIP_MESH_RENDER_PARITY_OUT")
    if out and _figures:
        with open(out, "w") as f:
            json.dump(_figures, f, indent=1, sort_keys=True)


def _ctx():
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
    ref_err = float(np.abs(np.asarray(f32, np.float64) - f64).max() / mx)
    err = float(np.abs(got - f64).max() / mx)
    bar = FACTOR * ref_err + FLOOR
    print("%s: kernel %.3e reference %.3e bar %.3e" % (name, err, ref_err, bar))
    _figures[name] = dict(kernel_err=err, reference_err=ref_err, bar=bar)
    assert err <= bar, (name, err, ref_err, bar)
    return bar


def _ids(rast):
    return _np(rast[..., 3]).astype(np.int64) - 1


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _counts():
    from gaussianip_amd import _lib
    return dict(_lib.call_counts)


def _launches(before):
    """The calls into the library since `before`."""
    after = _counts()
    return {k: after[k] - before.get(k, 0) for k in after if after[k] != before.get(k, 0)}


class _Cam:
    """What render_mesh reads of a camera."""

    def __init__(self, proj, h=H, w=W):
        self.full_proj_transform, self.image_height, self.image_width = _cu(proj), h, w


MIRROR = np.diag([-1, 1, 1, 1]).astype(np.float32)      # a second exact view: x mirrored


# ---------------------------------------------------------------------------------------------------------------- 1. coverage
@functools.lru_cache(maxsize=None)
def _coverage():
    pos, tri, tags = inputs.coverage_views()
    return pos, tri, tags, ref.rasterize(pos, tri, H, W), ref.rasterize(pos, tri, H, W, cull_backfaces=True)


def test_coverage_is_bit_exact():
    pos, tri, tags, want, culled = _coverage()
    ctx = _ctx()
    before = _counts()
    rast, db = ctx.rasterize(_cu(pos), _cu(tri), (H, W))
    assert db is None and _launches(before) == {"gip_mesh_rasterize": 1}
    assert rast.shape == (2, H, W, 4) and rast.dtype == torch.float32 and rast.is_cuda
    assert np.array_equal(_ids(rast), want["tri"])
    assert np.array_equal(_bits(_np(rast[..., 2])), _bits(want["depth"]))
    won = set(np.unique(_ids(rast)))
    assert all(t in won for t in tags["screen_filling"]) and tags["coincident"][0] in won and tags["coincident"][1] not in won
    again, _ = ctx.rasterize(_cu(pos), _cu(tri), (H, W))
    assert torch.equal(again, rast)
    back, _ = ctx.rasterize(_cu(pos), _cu(tri), (H, W), cull_backfaces=True)
    assert np.array_equal(_ids(back), culled["tri"]) and np.array_equal(_bits(_np(back[..., 2])), _bits(culled["depth"]))
    assert not np.array_equal(culled["tri"], want["tri"])


def test_the_grid_gives_every_pixel_one_owner():
    pos, tri = inputs.grid_views()
    want = ref.rasterize(pos, tri, H, W)
    assert (want["covering"] == 1).all()
    rast, _ = _ctx().rasterize(_cu(pos), _cu(tri), (H, W))
    assert np.array_equal(_ids(rast), want["tri"]) and (_ids(rast) >= 0).all()
    assert np.array_equal(_bits(_np(rast[..., 2])), _bits(want["depth"]))
    centred = inputs.grid_mesh(3, on_centres=True)
    rast, _ = _ctx().rasterize_one(_cu(centred[0]), _cu(centred[1]), (H, W))
    assert np.array_equal(_ids(rast), ref.rasterize(centred[0][None], centred[1], H, W)["tri"][0]) and (_ids(rast) >= 0).all()


# ---------------------------------------------------------------------------------------------------------------- 2. barycentrics
@functools.lru_cache(maxsize=None)
def _grid():
    """The jittered grid under its strongly perspective views: w spans 1 : 20."""
    pos, tri = inputs.grid_views()
    assert pos[..., 3].max() / pos[..., 3].min() > 15
    ids = ref.rasterize(pos, tri, H, W)["tri"]
    return pos, tri, ids, ref.barycentrics(pos, tri, H, W, ids, np.float64), ref.barycentrics(pos, tri, H, W, ids, np.float32)


def test_barycentrics_and_interpolation():
    pos, tri, ids, b64, b32 = _grid()
    ctx = _ctx()
    rast, _ = ctx.rasterize(_cu(pos), _cu(tri), (H, W))
    assert np.array_equal(_ids(rast), ids)
    bar = _rule("u", _np(rast[..., 0]), b64[0], b32[0])
    _rule("v", _np(rast[..., 1]), b64[1], b32[1])
    _rule("depth", _np(rast[..., 2]), b64[2], b32[2])
    flat = ref.barycentrics(pos, tri, H, W, ids, np.float64, perspective=False)
    assert np.abs(flat[0] - b64[0]).max() > 1000 * bar              # screen-space interpolation is nowhere near
    rng = np.random.default_rng(3)
    attr = rng.normal(size=(pos.shape[1], 5)).astype(np.float32)
    own_idx = rng.integers(0, 40, (len(tri), 3)).astype(np.int32)
    own_attr = rng.normal(size=(2, 40, 5)).astype(np.float32)        # one set of rows per view, indexed by its own tensor
    before = _counts()
    out, none = ctx.interpolate(_cu(attr), rast, _cu(tri))
    assert none is None and out.shape == (2, H, W, 5) and _launches(before) == {"gip_mesh_interpolate": 1}
    _rule("interpolate_shared_index", _np(out), ref.interpolate(attr, tri, ids, b64[0], b64[1], np.float64),
          ref.interpolate(attr, tri, ids, b32[0], b32[1], np.float32))
    out, _ = ctx.interpolate(_cu(own_attr), rast, _cu(own_idx))
    _rule("interpolate_own_index", _np(out), ref.interpolate(own_attr, own_idx, ids, b64[0], b64[1], np.float64),
          ref.interpolate(own_attr, own_idx, ids, b32[0], b32[1], np.float32))
    one, _ = ctx.interpolate_one(_cu(attr), rast, _cu(tri))
    assert torch.equal(one, ctx.interpolate(_cu(attr), rast, _cu(tri))[0])


# ---------------------------------------------------------------------------------------------------------------- 3. lookup and shade
def _shade_case(T, seed):
    """The grid seen by two exact cameras (inputs.EXACT_PROJ and its mirror image), a random T x T texture and OBJ texture coordinates:
    the atlas of the 96 faces for T = 32, arbitrary ones reaching outside [0, 1] for T = 5."""
    from gaussianip_amd.utils import texture as atlas
    rng = np.random.default_rng(seed)
    clip, tri = inputs.grid_mesh(1000)
    world = inputs.world_of(clip)
    pos = np.stack((inputs.exact_clip(world), inputs.exact_clip(world) * np.array([-1, 1, 1, 1], np.float32)))
    uv = atlas.atlas_uv(len(tri), T) if T == 32 else rng.uniform(-0.5, 1.5, (len(tri), 3, 2)).astype(np.float32)
    tex = rng.uniform(0, 1, (T, T, 3)).astype(np.float32)
    bg = np.array([0.25, 0.5, 0.75], np.float32)
    ids = ref.rasterize(pos, tri, H, W)["tri"]
    flipped = np.stack((uv[..., 0], np.float32(1) - uv[..., 1]), -1)           # float32, as render_mesh flips it
    b64, b32 = ref.barycentrics(pos, tri, H, W, ids, np.float64), ref.barycentrics(pos, tri, H, W, ids, np.float32)
    return dict(world=world, pos=pos, tri=tri, uv=uv, flipped=flipped, tex=tex, bg=bg, ids=ids, b64=b64, b32=b32,
                cams=[_Cam(inputs.EXACT_PROJ), _Cam(MIRROR @ inputs.EXACT_PROJ)])


@functools.lru_cache(maxsize=None)
def _shade_cases():
    return {32: _shade_case(32, 11), 5: _shade_case(5, 12)}


@pytest.mark.parametrize("T", [32, 5])
def test_fused_shade(T):
    from gaussianip_amd.utils.rasterize import render_mesh
    c = _shade_cases()[T]
    ctx = _ctx()
    args = (_cu(c["world"]), _cu(c["tri"]), _cu(c["uv"]), _cu(c["tex"]))
    before = _counts()
    out = render_mesh(c["cams"], *args, bg_color=_cu(c["bg"]))       # the first render of this shape in the process
    assert _launches(before) == {"gip_mesh_rasterize": 1, "gip_mesh_shade": 1}
    assert set(out) == {"image", "alpha", "depth", "rast"}
    assert out["image"].shape == (2, 3, H, W) and out["alpha"].shape == (2, 1, H, W) and out["depth"].shape == (2, 1, H, W)
    # render_mesh rasterized exactly the positions this test knows
    rast, _ = ctx.rasterize(_cu(c["pos"]), _cu(c["tri"]), (H, W))
    assert torch.equal(out["rast"], rast) and np.array_equal(_ids(rast), c["ids"])
    assert (c["ids"] >= 0).all() and len(np.unique(c["ids"])) > 60
    col64, a64 = ref.shade(c["tex"], c["flipped"], c["ids"], c["b64"][0], c["b64"][1], c["bg"], np.float64)
    col32, _ = ref.shade(c["tex"], c["flipped"], c["ids"], c["b32"][0], c["b32"][1], c["bg"], np.float32)
    image = _np(out["image"]).transpose(0, 2, 3, 1)
    bar = _rule("shade_T%d_colour" % T, image, col64, col32)
    assert np.array_equal(_np(out["alpha"])[:, 0], a64)
    _rule("shade_T%d_depth" % T, _np(out["depth"])[:, 0], c["b64"][2], c["b32"][2])
    if T == 5:
        st = ref.interpolate(c["flipped"].reshape(-1, 2), np.arange(len(c["tri"]) * 3).reshape(-1, 3), c["ids"], c["b64"][0], c["b64"][1],
                             np.float64)
        assert st.min() < -0.1 and st.max() > 1.1                    # lookups beyond the border: clamped
    # the unfused chain: rasterize -> interpolate -> texture -> composite
    corner = _cu(np.arange(len(c["tri"]) * 3, dtype=np.int32).reshape(-1, 3))
    st, _ = ctx.interpolate(_cu(c["flipped"].reshape(-1, 2)), rast, corner)
    looked = ctx.texture(_cu(c["tex"])[None], st)
    chain = torch.where(rast[..., 3:] > 0, looked, _cu(c["bg"]))
    _rule("chain_T%d_colour" % T, _np(chain), col64, col32)
    assert float((chain - out["image"].permute(0, 2, 3, 1)).abs().max()) <= bar * float(np.abs(col64).max())
    # one camera, not a list: no leading dimension
    single = render_mesh(c["cams"][1], *args, bg_color=c["bg"])
    assert single["image"].shape == (3, H, W) and torch.equal(single["image"], out["image"][1]) and torch.equal(single["rast"], rast[1])


def test_texture_lookup():
    rng = np.random.default_rng(21)
    tex = rng.normal(size=(2, 5, 7, 4)).astype(np.float32)             # a texture per view, not square, four channels
    uv = rng.uniform(-0.5, 1.5, (2, 9, 11, 2)).astype(np.float32)
    uv[0, 0, :2] = [[0, 0], [1, 1]]                                    # the texture's corners: half a texel beyond the last centre
    out = _ctx().texture(_cu(tex), _cu(uv))
    want64 = np.stack([ref.texture(tex[b], uv[b], np.float64) for b in range(2)])
    want32 = np.stack([ref.texture(tex[b], uv[b], np.float32) for b in range(2)])
    _rule("texture_lookup", _np(out), want64, want32)
    assert np.array_equal(_np(out)[0, 0, :2], tex[0][[0, 4], [0, 6]])   # clamped: the corner texel itself, exactly
    shared = _ctx().texture(_cu(tex[1]), _cu(uv))                      # [Th, Tw, C]: one texture for every view
    assert torch.equal(shared[1], out[1])


# ---------------------------------------------------------------------------------------------------------------- 4. gradients
@pytest.mark.parametrize("T", [32, 5])
def test_gradients_of_the_fused_shade(T):
    from gaussianip_amd.utils.rasterize import render_mesh
    c = _shade_cases()[T]
    F = len(c["tri"])
    g = np.random.default_rng(40 + T).normal(size=(2, H, W, 3)).astype(np.float32)
    tex, uv = _cu(c["tex"]).requires_grad_(True), _cu(c["uv"]).requires_grad_(True)
    before = _counts()
    out = render_mesh(c["cams"], _cu(c["world"]), _cu(c["tri"]), uv, tex, bg_color=c["bg"])
    (out["image"] * _cu(g).permute(0, 3, 1, 2)).sum().backward()
    assert _launches(before) == {"gip_mesh_rasterize": 1, "gip_mesh_shade": 1, "gip_mesh_shade_backward": 1}
    corner = np.arange(F * 3).reshape(F, 3)
    want, touched = {}, np.zeros((T, T), bool)
    for dt in (np.float64, np.float32):
        u, v = c["b64" if dt is np.float64 else "b32"][:2]
        st = ref.interpolate(c["flipped"].reshape(-1, 2), corner, c["ids"], u, v, dt)
        g_tex, g_st = ref.texture_grad(c["tex"], st, g, c["ids"] >= 0, dt)
        g_uv = ref.interpolate_grad((F * 3, 2), corner, c["ids"], u, v, g_st, dt).reshape(F, 3, 2) * np.array([1, -1], dt)      # the flip
        want[dt] = (g_tex, g_uv)
        x0, x1, y0, y1, _, _ = ref.lookup_setup(st, T, T, dt)
        for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)):
            touched[yy, xx] = True
    bar_tex = _rule("grad_T%d_texture" % T, _np(tex.grad), want[np.float64][0], want[np.float32][0])
    _rule("grad_T%d_uv" % T, _np(uv.grad), want[np.float64][1], want[np.float32][1])
    assert not _np(tex.grad)[~touched].any()                          # exactly 0 where no visible pixel reaches
    if T == 32:
        assert (~touched).sum() > 50
    # Linearity in the texture: <p, render(tex)> - <p, render(0)> = <dL/dtex, tex>, to the bar relative to the value.  The upstream
    # gradient p of this check is random in (0.5, 1.5): with a positive one the inner product is a sum of terms of one sign, so a bar
    # relative to it means what it says (the normal g above sums 18090 terms to a value a hundred times smaller than their
    # magnitudes' sum, and its sign and size are an accident of the seed).  The left side carries the colour's error, the right side
    # the gradient's: the bar is the sum of the two bars of the rule.
    p = np.random.default_rng(60 + T).uniform(0.5, 1.5, size=(2, H, W, 3)).astype(np.float32)
    tex.grad = None
    again = render_mesh(c["cams"], _cu(c["world"]), _cu(c["tri"]), uv.detach(), tex, bg_color=c["bg"])
    (again["image"] * _cu(p).permute(0, 3, 1, 2)).sum().backward()
    with torch.no_grad():
        zero = render_mesh(c["cams"], _cu(c["world"]), _cu(c["tri"]), uv.detach(), torch.zeros_like(tex), bg_color=c["bg"])
    img, img0 = (_np(o["image"]).transpose(0, 2, 3, 1).astype(np.float64) for o in (again, zero))
    lhs = float((p * (img - img0)).sum())
    rhs = float((_np(tex.grad).astype(np.float64) * c["tex"]).sum())
    col64, _ = ref.shade(c["tex"], c["flipped"], c["ids"], c["b64"][0], c["b64"][1], c["bg"], np.float64)
    col32, _ = ref.shade(c["tex"], c["flipped"], c["ids"], c["b32"][0], c["b32"][1], c["bg"], np.float32)
    bar_col = FACTOR * float(np.abs(col32 - col64).max() / np.abs(col64).max()) + FLOOR
    bar = bar_col + bar_tex
    err = abs(lhs - rhs) / abs(lhs)
    print("linearity T%d: %.9g vs %.9g, relative difference %.3e, bar %.3e" % (T, lhs, rhs, err, bar))
    _figures["linearity_T%d" % T] = dict(lhs=lhs, rhs=rhs, relative_difference=err, bar=bar)
    assert err <= bar


def test_gradients_of_interpolate_and_texture():
    pos, tri, ids, b64, b32 = _grid()
    ctx = _ctx()
    rng = np.random.default_rng(50)
    rast, _ = ctx.rasterize(_cu(pos), _cu(tri), (H, W))
    attr = _cu(rng.normal(size=(pos.shape[1], 5)).astype(np.float32)).requires_grad_(True)
    g = rng.normal(size=(2, H, W, 5)).astype(np.float32)
    out, _ = ctx.interpolate(attr, rast, _cu(tri))
    (out * _cu(g)).sum().backward()
    _rule("grad_interpolate", _np(attr.grad), ref.interpolate_grad(tuple(attr.shape), tri, ids, b64[0], b64[1], g, np.float64),
          ref.interpolate_grad(tuple(attr.shape), tri, ids, b32[0], b32[1], g, np.float32))
    used = np.zeros(pos.shape[1], bool)
    used[tri[np.unique(ids)].ravel()] = True
    assert not _np(attr.grad)[~used].any()
    tex_np = rng.normal(size=(5, 5, 3)).astype(np.float32)
    uv_np = rng.uniform(-0.5, 1.5, (2, 9, 11, 2)).astype(np.float32)
    g = rng.normal(size=(2, 9, 11, 3)).astype(np.float32)
    tex, uv = _cu(tex_np).requires_grad_(True), _cu(uv_np).requires_grad_(True)
    (ctx.texture(tex, uv) * _cu(g)).sum().backward()
    everywhere = np.ones(uv_np.shape[:3], bool)
    w64, w32 = (ref.texture_grad(tex_np, uv_np, g, everywhere, dt) for dt in (np.float64, np.float32))
    _rule("grad_texture_tex", _np(tex.grad), w64[0], w32[0])
    _rule("grad_texture_uv", _np(uv.grad), w64[1], w32[1])


# ---------------------------------------------------------------------------------------------------------------- 5. extremes
def test_no_faces():
    from gaussianip_amd.utils.rasterize import render_mesh
    ctx = _ctx()
    none = torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    before = _counts()
    rast, _ = ctx.rasterize(torch.zeros((2, 4, 4), device="cuda"), none, (H, W))
    assert rast.shape == (2, H, W, 4) and not rast.any() and _launches(before) == {}
    tex = torch.rand((8, 8, 3), device="cuda").requires_grad_(True)
    bg = torch.tensor([0.1, 0.2, 0.3], device="cuda")
    out = render_mesh(_Cam(inputs.EXACT_PROJ), torch.zeros((0, 3), device="cuda"), none, torch.zeros((0, 3, 2), device="cuda"), tex, bg_color=bg)
    assert "gip_mesh_rasterize" not in _launches(before)
    assert torch.equal(out["image"], bg[:, None, None].expand(3, H, W)) and not out["alpha"].any() and not out["depth"].any()
    out["image"].sum().backward()
    assert tex.grad is not None and not tex.grad.any()


@pytest.mark.parametrize("h,w", [(1, 1), (H, W)])
def test_one_face(h, w):
    pos = np.array([[[-4, -3, 0.25, 1], [8, -6, 1.0, 2], [0, 7.5, -0.5, 1.5]]], np.float32)      # NDC (-4, -3), (4, -3), (0, 5): the whole image
    tri = np.array([[0, 1, 2]], np.int32)
    ctx = _ctx()
    rast, _ = ctx.rasterize(_cu(pos), _cu(tri), (h, w))
    want = ref.rasterize(pos, tri, h, w)
    assert (want["tri"] == 0).all() and np.array_equal(_ids(rast), want["tri"]) and np.array_equal(_bits(_np(rast[..., 2])), _bits(want["depth"]))
    b64, b32 = ref.barycentrics(pos, tri, h, w, want["tri"], np.float64), ref.barycentrics(pos, tri, h, w, want["tri"], np.float32)
    _rule("one_face_%dx%d_u" % (h, w), _np(rast[..., 0]), b64[0], b32[0])
    one, _ = ctx.rasterize_one(_cu(pos[0]), _cu(tri), (h, w))          # B = 1 as [V, 4]
    assert one.shape == (h, w, 4) and torch.equal(one, rast[0])
    part = pos.copy()
    part[0, :, :2] = [[0.9, 0.9], [0.95, 0.9], [0.9, 0.95]]            # NDC (0.9, 0.9), (0.475, 0.45), (0.6, 0.633): most pixels stay empty
    rast, _ = ctx.rasterize(_cu(part), _cu(tri), (h, w))
    want = ref.rasterize(part, tri, h, w)
    assert (want["tri"] < 0).any()
    assert np.array_equal(_ids(rast), want["tri"]) and not rast[rast[..., 3] == 0].any()


def test_resolution_as_an_int_and_argument_errors():
    from gaussianip_amd.utils.rasterize import render_mesh
    pos, tri = inputs.grid_views()
    ctx = _ctx()
    p, t = _cu(pos), _cu(tri)
    rast, _ = ctx.rasterize(p, t, 24)
    assert rast.shape == (2, 24, 24, 4) and np.array_equal(_ids(rast), ref.rasterize(pos, tri, 24, 24)["tri"])
    for bad_pos, bad_tri in ((p.cpu(), t), (p, t.cpu()), (p.double(), t), (p, t.long()), (p[0], t), (p[..., :3], t), (p, t[:, :2])):
        with pytest.raises(ValueError):
            ctx.rasterize(bad_pos, bad_tri, (H, W))
    for value in (pos.shape[1], -1):
        bad = t.clone()
        bad[5, 2] = value
        with pytest.raises(ValueError, match="indices"):
            ctx.rasterize(p, bad, (H, W))
    for resolution in (0, (4, 0), (1, 2, 3), 20000):
        with pytest.raises(ValueError):
            ctx.rasterize(p, t, resolution)
    attr = torch.zeros((pos.shape[1], 3), device="cuda")
    with pytest.raises(ValueError, match="indices"):
        ctx.interpolate(attr[:10], rast, t)
    with pytest.raises(ValueError):
        ctx.interpolate(attr.double(), rast, t)
    with pytest.raises(ValueError):
        ctx.texture(torch.zeros((3, 4, 4, 3), device="cuda"), torch.zeros((2, 4, 4, 2), device="cuda"))      # a batch of 3 for 2 views
    # what is out of scope says so, naming the argument
    with pytest.raises(NotImplementedError, match="rast_db"):
        ctx.interpolate(attr, rast, t, rast_db=rast)
    with pytest.raises(NotImplementedError, match="diff_attrs"):
        ctx.interpolate(attr, rast, t, diff_attrs="all")
    with pytest.raises(NotImplementedError, match="filter_mode"):
        ctx.texture(torch.zeros((1, 4, 4, 3), device="cuda"), torch.zeros((2, 4, 4, 2), device="cuda"), filter_mode="linear-mipmap-linear")
    with pytest.raises(NotImplementedError, match="antialias"):
        ctx.antialias(rast, rast, p, t)
    with pytest.raises(NotImplementedError, match="pos"):
        ctx.rasterize(p.clone().requires_grad_(True), t, (H, W))
    world = _cu(inputs.world_of(pos[0]))
    uv, tex = torch.zeros((len(tri), 3, 2), device="cuda"), torch.zeros((8, 8, 3), device="cuda")
    with pytest.raises(NotImplementedError, match="vertices"):
        render_mesh(_Cam(inputs.EXACT_PROJ), world.clone().requires_grad_(True), t, uv, tex)
    for args in ((world, t, uv[:5], tex), (world, t, uv, tex[..., :2]), (world.cpu(), t, uv, tex), (world, t, uv, tex.cpu())):
        with pytest.raises(ValueError):
            render_mesh(_Cam(inputs.EXACT_PROJ), *args)
    clip = ctx.vertex_transform(world, _cu(np.stack((inputs.EXACT_PROJ.T, (MIRROR @ inputs.EXACT_PROJ).T))))      # column-vector matrices
    assert clip.shape == (2, pos.shape[1], 4) and np.array_equal(_np(clip[0]), inputs.exact_clip(_np(world)))
    assert np.array_equal(_np(clip[1]), inputs.exact_clip(_np(world)) * np.array([-1, 1, 1, 1], np.float32))
    # validate=False: no host read, and a triangle with an index out of range is dropped by the kernels
    bad = t.clone()
    bad[5, 2] = pos.shape[1]
    rast, _ = ctx.rasterize(p, bad, (H, W), validate=False)
    want = ref.rasterize(pos, _np(bad), H, W)["tri"]
    assert np.array_equal(_ids(rast), want) and not (want == 5).any() and (want < 0).any()


# ---------------------------------------------------------------------------------------------------------------- 6. end to end
def _model(cl, colors=None):
    from gaussianip_amd.scene import GaussianModel
    from gaussianip_amd.utils.sh import C0
    gm = GaussianModel(0)
    gm._xyz, gm._opacity = _cu(cl["xyz"]), _cu(cl["opacity"])
    gm._scaling, gm._rotation = _cu(cl["scaling"]), _cu(cl["rotation"])
    P = cl["xyz"].shape[0]
    rgb = np.full((P, 3), 0.5, np.float32) if colors is None else colors
    gm._features_dc = ((_cu(rgb) - 0.5) / C0).reshape(P, 1, 3).contiguous()
    gm._features_rest = torch.zeros((P, 0, 3), device="cuda")
    return gm


def _camera(el, az, dist, target, fovy_deg, size):
    """A camera of the project on the orbit of scenes.orbit_c2w, moved so that `target` lands on the image centre at depth `dist`.
    Camera negates rows 1-2 of the world-to-camera rotation and its whole translation (x_cam = D R x + R pos, R the transposed
    rotation of c2w, D = diag(1, -1, -1)), so the move of the camera that does this is -R^T D R target."""
    from gaussianip_amd.scene import Camera
    c2w = scenes.orbit_c2w(el, az, dist)
    rot = c2w[:3, :3].clone()
    c2w[:3, 3] -= rot @ torch.diag(torch.tensor([1.0, -1.0, -1.0])) @ rot.t() @ torch.tensor(target, dtype=torch.float32)
    return Camera(c2w=c2w.cuda(), FoVy=math.radians(fovy_deg), height=size, width=size)


def test_sphere_end_to_end():
    """One isotropic Gaussian extracted at resolution 32 and rendered from a short orbit at 96 x 96, the cameras looking at its centre
    from a distance of 3 with a field of view of 20 degrees: the sphere's radius is about 15 pixels.

    The depth at the image centre is compared with the analytic sphere's front, dist - SPHERE_RADIUS along the axis.  The mesh is not
    the sphere: a flat face across a grid cell (h = 2 / 31 / 1.8 = 0.036 world units) lies up to h^2 / (8 r) = 1e-3 inside it, and the
    linear interpolation of the crossings moves a vertex by about 2e-4.  In z/w = zfar (z - znear) / (z (zfar - znear)) a distance error
    e costs znear e / z^2 = 0.01 * 1.2e-3 / 2.84^2 = 1.5e-6; that is why the orbit is this far out: at a distance of 1.5 the same face
    would cost 7e-6, above the bar, with nothing wrong in the rasterizer."""
    from gaussianip_amd.utils.rasterize import render_mesh
    cl, rgb = sample_inputs.sphere_cloud()
    gm = _model(cl, rgb)
    v, f, _, uv, texture = gm.extract_textured_mesh(density_thresh=sample_inputs.SPHERE_THRESHOLD, resolution=32, num_blocks=4)
    size, dist = 96, 3.0
    cams = [_camera(10.0 + 5 * i, 20.0 + 25 * i, dist, sample_inputs.SPHERE_MU, 20.0, size) for i in range(3)]
    out = render_mesh(cams, v, f, uv, texture, bg_color=[1.0, 1.0, 1.0])
    alpha = _np(out["alpha"])[:, 0]
    image = _np(out["image"]).transpose(0, 2, 3, 1)
    colour_err = np.abs(image[alpha > 0] - np.array(sample_inputs.SPHERE_COLOR, np.float32)).max()
    print("%d faces, texture %d, %s covered pixels, colour error %.3e" % (f.shape[0], texture.shape[0], alpha.sum((1, 2)), colour_err))
    _figures["sphere_colour_err"] = float(colour_err)
    assert colour_err <= 1e-5
    assert (image[alpha == 0] == 1).all()
    for b in range(3):
        assert 400 < alpha[b].sum() < 1200                            # a disc of radius about 15 pixels
        for row in alpha[b]:
            xs = np.nonzero(row)[0]
            assert len(xs) == 0 or len(xs) == xs[-1] - xs[0] + 1      # filled: a row's covered pixels are contiguous
    # the depth at the image centre (the four pixels around it) against the sphere's front
    z = dist - sample_inputs.SPHERE_RADIUS
    znear, zfar = cams[0].znear, cams[0].zfar
    front = zfar * (z - znear) / (z * (zfar - znear))
    centre = _np(out["depth"])[:, 0, size // 2 - 1:size // 2 + 1, size // 2 - 1:size // 2 + 1]
    pos = _np(torch.matmul(torch.cat((v, torch.ones_like(v[:, :1])), 1)[None], torch.stack([c.full_proj_transform for c in cams])))
    ids = _ids(out["rast"])
    d64, d32 = (ref.barycentrics(pos, _np(f), size, size, ids, dt)[2] for dt in (np.float64, np.float32))
    bar = _rule("sphere_depth", _np(out["depth"])[:, 0], d64, d32)
    err = float(np.abs(centre - front).max() / np.abs(d64).max())
    print("depth at the centre %s, the sphere's front %.8f: error %.3e, bar %.3e" % (centre.ravel()[:4], front, err, bar))
    _figures["sphere_front_depth"] = dict(err=err, bar=bar)
    assert err <= bar


def test_alignment_with_the_gaussian_render():
    """The exported mesh lands on the Gaussian render of the same camera: the centroids of the two alpha images agree to a pixel.  A
    flipped axis or a half-pixel shift of the pixel grid would move them apart; the camera looks past the blob so that it sits away
    from the image centre.  The PSNR between the two images is printed, without a bar: it measures the baked texture."""
    from gaussianip_amd.arguments import PipelineParams
    from gaussianip_amd.renderer import render
    cl = sample_inputs.blob_cloud()
    rgb = sample_inputs.colors(cl["xyz"].shape[0], 9)
    gm = _model(cl, rgb)
    size = 128
    cam = _camera(20.0, 35.0, 2.2, (0.15, -0.2, 0.25), 50.0, size)
    bg = torch.zeros(3, device="cuda")
    with torch.no_grad():
        pkg = render(cam, gm, PipelineParams(ArgumentParser()), bg)
    mesh = gm.render_textured_mesh(cam, bg_color=bg, density_thresh=1.0, resolution=64, num_blocks=8)
    assert set(mesh) == {"image", "alpha", "depth", "rast", "mesh"} and mesh["image"].shape == (3, size, size)
    ys, xs = np.mgrid[0:size, 0:size]
    centroid = lambda a: np.array([(a * xs).sum(), (a * ys).sum()]) / a.sum()  # noqa: E731
    cg, cm = centroid(_np(pkg["alpha_3dgs"])[0].astype(np.float64)), centroid(_np(mesh["alpha"])[0].astype(np.float64))
    mse = float(((pkg["render"] - mesh["image"]) ** 2).mean())
    psnr = 10 * math.log10(1 / mse)
    print("centroids: Gaussians (%.2f, %.2f), mesh (%.2f, %.2f); %d faces; PSNR %.2f dB" % (cg[0], cg[1], cm[0], cm[1], mesh["mesh"][1].shape[0], psnr))
    _figures["alignment"] = dict(gaussians=cg.tolist(), mesh=cm.tolist(), psnr_db=psnr)
    record = os.environ.get("GIP_MESH_RENDER_PROFILE_OUT")             # profiles/mesh_render.json on a recording run: the PSNR joins it
    if record and os.path.exists(record):
        with open(record) as fh:
            profile = json.load(fh)
        profile["alignment_test_128"] = dict(_figures["alignment"], scene="blob_cloud at resolution 64, 128 x 128, this test")
        with open(record, "w") as fh:
            fh.write(json.dumps(profile, indent=1, sort_keys=True) + "\n")
    assert np.abs(cg - np.array([size / 2 - 0.5] * 2)).min() > 5        # off-centre on both axes: a flip would show
    assert np.abs(cg - cm).max() <= 1.0
