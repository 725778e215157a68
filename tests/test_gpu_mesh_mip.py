"""Pixel differentials and the mipmapped lookup on the GPU (csrc/mesh_mip.hip, MipMeshRasterizerContext of
gaussianip_amd/utils/rasterize.py) against tests/mesh_mip_reference.py, the definition restated in numpy.

The comparison rule is that of tests/test_gpu_mesh_render.py: errors normalised by the output's maximum, at most 4 times the float32
error of the restatement against itself in float64 plus a floor of 2e-6; the restatement's error is computed here and printed.  The
mip build is compared bit for bit: it is the same additions in the same order.  Decisions (which two levels a pixel reads, whether its
level is clamped) are kept away from their thresholds by construction, and the tests assert that on the float64 restatement.

With GIP_MESH_MIP_PARITY_OUT=<file> the figures are written there as JSON (profiles/mesh_mip_parity.json is such a run)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import mesh_grad_inputs as scenes
import mesh_mip_reference as mref
import mesh_render_inputs as inputs
import mesh_render_reference as ref

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 4.0, 2e-6
H, W = inputs.H, inputs.W
F32, F64 = np.float32, np.float64
_figures = {}


@pytest.fixture(scope="module", autouse=True)
def _write_figures():
    yield
    out = os.environ.get("GIP_MESH_MIP_PARITY_OUT")
    if out and _figures:
        with open(out, "w") as f:
            json.dump(_figures, f, indent=1, sort_keys=True)


def _ctx():
    from gaussianip_amd.utils.rasterize import MipMeshRasterizerContext
    return MipMeshRasterizerContext()


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _rule(name, got, f64, f32):
    """The rule of the module's docstring; returns the bar (relative to the output's maximum)."""
    got, f64 = np.asarray(got, np.float64), np.asarray(f64, np.float64)
    assert got.shape == f64.shape, (name, got.shape, f64.shape)
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


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _counts():
    from gaussianip_amd import _lib
    return dict(_lib.call_counts)


def _launches(before):
    """The calls into the library since `before`."""
    after = _counts()
    return {k: after[k] - before.get(k, 0) for k in after if after[k] != before.get(k, 0)}


# ---------------------------------------------------------------------------------------------------------------- 1. rast_db
@functools.lru_cache(maxsize=None)
def _scene(name):
    """The jittered grid under its strongly perspective views (w spans 1 : 20, every pixel covered), or the silhouette scene (empty
    pixels), with the restatement's barycentrics and rast_db in both precisions."""
    pos, tri = inputs.grid_views() if name == "grid" else scenes.silhouette_views()
    ids = ref.rasterize(pos, tri, H, W)["tri"]
    b64, b32 = ref.barycentrics(pos, tri, H, W, ids, F64), ref.barycentrics(pos, tri, H, W, ids, F32)
    db64 = mref.rast_db(pos, tri, H, W, ids, b64[0], b64[1], F64)
    db32 = mref.rast_db(pos, tri, H, W, ids, b32[0], b32[1], F32)
    return dict(pos=pos, tri=tri, ids=ids, b64=b64, b32=b32, db64=db64, db32=db32)


@pytest.mark.parametrize("name", ["grid", "silhouette"])
def test_rast_db(name):
    from gaussianip_amd.utils.rasterize import DiffMeshRasterizerContext, MeshRasterizerContext
    s = _scene(name)
    pos, tri, ids = s["pos"], s["tri"], s["ids"]
    if name == "grid":
        assert pos[..., 3].max() / pos[..., 3].min() > 15 and (ids >= 0).all()
    else:
        assert (ids < 0).sum() > 200 and len(np.unique(ids)) >= 8
    ctx = _ctx()
    p, t = _cu(pos), _cu(tri)
    before = _counts()
    rast, db = ctx.rasterize(p, t, (H, W))
    assert _launches(before) == {"gip_mesh_rasterize": 1, "gip_mesh_rast_db": 1}
    assert db.shape == (2, H, W, 4) and db.dtype == torch.float32 and db.is_cuda and not db.requires_grad
    base, none = MeshRasterizerContext().rasterize(p, t, (H, W))
    assert none is None and torch.equal(rast, base)
    assert np.array_equal(_np(rast[..., 3]).astype(np.int64) - 1, ids)
    _rule("rast_db_%s" % name, _np(db), s["db64"], s["db32"])
    assert not _np(db)[ids < 0].any()                                  # exactly 0 at empty pixels
    assert np.abs(s["db64"]).max(-1)[ids >= 0].min() > 0               # and nowhere else
    one_rast, one_db = ctx.rasterize_one(p[1], t, (H, W))
    assert one_db.shape == (H, W, 4) and torch.equal(one_db, db[1]) and torch.equal(one_rast, rast[1])
    # gradients to positions go through rast as in the parent class; rast_db carries none
    g = _cu(np.random.default_rng(1).normal(size=(2, H, W, 4)).astype(np.float32))
    grads = []
    for c in (ctx, DiffMeshRasterizerContext()):
        q = p.clone().requires_grad_(True)
        out = c.rasterize(q, t, (H, W))
        assert out[0].requires_grad and (out[1] is None or not out[1].requires_grad)
        (out[0] * g).sum().backward()
        grads.append(_np(q.grad))
    assert np.abs(grads[0]).max() > 0 and np.abs(grads[0] - grads[1]).max() <= 1e-5 * np.abs(grads[1]).max()


# ---------------------------------------------------------------------------------------------------------------- 2. attribute differentials
@pytest.mark.parametrize("diff_attrs,batch,own", [("all", 1, False), ([2, 0], 2, True), ("all", 2, True), ([2, 0], 1, False)])
def test_interpolate_with_diff_attrs(diff_attrs, batch, own):
    s = _scene("silhouette" if own else "grid")
    pos, tri, ids = s["pos"], s["tri"], s["ids"]
    rng = np.random.default_rng(10 + batch)
    N, C = (60, 5) if own else (pos.shape[1], 5)
    idx = rng.integers(0, N, (len(tri), 3)).astype(np.int32) if own else tri          # an attribute's own index tensor, or the mesh's
    attr_np = rng.normal(size=((batch, N, C) if batch > 1 else (N, C))).astype(np.float32)
    channels = None if diff_attrs == "all" else diff_attrs
    K = C if channels is None else len(channels)
    ctx = _ctx()
    rast, db = ctx.rasterize(_cu(pos), _cu(tri), (H, W))
    attr = _cu(attr_np).requires_grad_(True)
    before = _counts()
    out, out_da = ctx.interpolate(attr, rast, _cu(idx), rast_db=db, diff_attrs=diff_attrs)
    assert _launches(before) == {"gip_mesh_interpolate": 1, "gip_mesh_interpolate_da": 1}
    plain, none = ctx.interpolate(attr, rast, _cu(idx))
    assert none is None and torch.equal(out, plain)                    # bit for bit the call without differentials
    assert out_da.shape == (2, H, W, 2 * K)
    tag = "%s_batch%d_%s" % ("all" if channels is None else "listed", batch, "own" if own else "tri")
    _rule("out_da_" + tag, _np(out_da), mref.interpolate_da(attr_np, idx, ids, s["db64"], channels, F64),
          mref.interpolate_da(attr_np, idx, ids, s["db32"], channels, F32))
    assert not _np(out_da)[ids < 0].any()
    g = rng.normal(size=(2, H, W, 2 * K)).astype(np.float32)
    (out_da * _cu(g)).sum().backward()
    _rule("grad_out_da_" + tag, _np(attr.grad), mref.interpolate_da_grad(attr_np.shape, idx, ids, s["db64"], channels, g, F64),
          mref.interpolate_da_grad(attr_np.shape, idx, ids, s["db32"], channels, g, F32))
    used = np.zeros((2, N), bool)
    for b in range(2):
        used[b, idx[np.unique(ids[b][ids[b] >= 0])].ravel()] = True
    unused = ~used if batch > 1 else ~used.any(0)
    assert not _np(attr.grad)[unused].any()                            # exactly 0 at rows no visible triangle names
    if own:
        assert unused.sum() > 5
    if channels is not None:
        assert not _np(attr.grad)[..., [1, 3, 4]].any()                # and at channels that are not listed
    one = ctx.interpolate_one(attr.detach() if batch == 1 else attr.detach()[0], rast, _cu(idx), db, diff_attrs)
    if batch == 1:
        assert torch.equal(one[1], out_da)


# ---------------------------------------------------------------------------------------------------------------- 3. the mip build
@pytest.mark.parametrize("shape,cap,L", [((16, 8, 3), None, 4), ((12, 20, 2), None, 2), ((1, 8, 1), None, 3), ((7, 7, 3), None, 0),
                                         ((16, 16, 3), 1, 1)])
def test_mip_build_is_bit_exact(shape, cap, L):
    rng = np.random.default_rng(sum(shape))
    tex = rng.normal(size=(2,) + shape).astype(np.float32)             # two textures: the batch stride is exercised
    ctx = _ctx()
    before = _counts()
    stack = ctx.texture_construct_mip(_cu(tex), max_mip_level=cap)
    assert _launches(before) == ({"gip_mesh_mip_levels": 1, "gip_mesh_mip_build": 1} if L else {"gip_mesh_mip_levels": 1})
    assert stack.L == L == mref.mip_levels(shape[0], shape[1], cap)
    got = stack.levels(_cu(tex))
    assert len(got) == L + 1
    for b in range(2):
        want = mref.mip_build(tex[b], cap, F32)
        assert len(want) == L + 1
        for l in range(L + 1):
            assert got[l].shape[1:] == want[l].shape and np.array_equal(_bits(_np(got[l][b])), _bits(want[l])), (b, l)
    if shape == (12, 20, 2):
        assert tuple(got[-1].shape[1:3]) == (3, 5)
    single = ctx.texture_construct_mip(_cu(tex[1]), max_mip_level=cap)   # [Th, Tw, C]
    assert single.L == L and (L == 0 or torch.equal(single.buffer[0], stack.buffer[1]))


# ---------------------------------------------------------------------------------------------------------------- 4. the lookup
TH, TW, TC = 16, 8, 3          # L = 4: 16 x 8, 8 x 4, 4 x 2, 2 x 1, 1 x 1
PIX = (2, 9, 11)


def _ellipse_uv_da(rng, level, Th, Tw):
    """uv_da whose footprint in texels is an ellipse with a major axis of 2^level texels, a random minor axis and rotation."""
    major = 2.0 ** level
    minor, phi = major * rng.uniform(0.2, 1.0, level.shape), rng.uniform(0, 2 * np.pi, level.shape)
    c, s = np.cos(phi), np.sin(phi)
    return np.stack((c * major / Tw, -s * minor / Tw, s * major / Th, c * minor / Th), -1).astype(np.float32)


def _clear(level, L):
    """No level within 1e-3 of an integer or a half-integer (0 and L are integers): every decision is the same in both precisions."""
    assert np.abs(level * 2 - np.rint(level * 2)).min() > 2e-3
    return level


@functools.lru_cache(maxsize=None)
def _lookup_inputs(kind):
    """"spread": uv uniform in (-0.5, 1.5), levels spread over [-2, L + 2] with fractional parts in [0.05, 0.45] u [0.55, 0.95].
    "corner": uv in (0.05, 0.45), levels in (-1, 1) (below 2 with the bias): the footprints stay in one corner of the texture.
    The bias is an integer -1 .. 1 moved by 0.01 .. 0.04 either way, so a biased level keeps its distance from the thresholds."""
    L = mref.mip_levels(TH, TW)
    rng = np.random.default_rng(30 if kind == "spread" else 31)
    frac = rng.uniform(0.05, 0.45, PIX) + 0.5 * rng.integers(0, 2, PIX)
    if kind == "spread":
        uv = rng.uniform(-0.5, 1.5, PIX + (2,))
        level = rng.integers(-2, L + 2, PIX) + frac
        assert level.min() < -1.5 and level.max() > L + 1.5
    else:
        uv = rng.uniform(0.05, 0.45, PIX + (2,))
        level = rng.integers(-1, 1, PIX) + frac
    uv = uv.astype(np.float32)
    uv_da = _ellipse_uv_da(rng, level, TH, TW)
    bias = (rng.integers(-1, 2, PIX) + rng.uniform(0.01, 0.04, PIX) * rng.choice([-1, 1], PIX)).astype(np.float32)
    tex = rng.uniform(0, 1, (2, TH, TW, TC)).astype(np.float32)
    got = mref.lod(uv_da, None, TH, TW, PIX, F64)["level"]
    assert np.abs(got - level).max() < 1e-5                           # the major axis sets the level
    return dict(uv=uv, uv_da=uv_da, bias=bias, tex=tex, L=L)


def _levels_of(c, with_bias, with_da=True):
    return _clear(mref.lod(c["uv_da"] if with_da else None, c["bias"] if with_bias else None, TH, TW, PIX, F64)["level"], c["L"])


def _textures(c, per_view):
    return [c["tex"][b if per_view else 0] for b in range(PIX[0])]


def _want(c, per_view, with_bias, dtype, nearest=False, with_da=True):
    return np.stack([mref.texture_mip(mref.mip_build(t, None, dtype), c["uv"][b], c["uv_da"][b] if with_da else None,
                                      c["bias"][b] if with_bias else None, dtype, nearest) for b, t in enumerate(_textures(c, per_view))])


def _want_grad(c, per_view, with_bias, g, dtype, nearest=False):
    """(g_tex [2 or 1 x Th x Tw x C], g_uv, g_uv_da, g_bias, touched like g_tex without channels)."""
    parts = [mref.texture_mip_grad(mref.mip_build(t, None, dtype), c["uv"][b], c["uv_da"][b], c["bias"][b] if with_bias else None, g[b], dtype,
                                   nearest) for b, t in enumerate(_textures(c, per_view))]
    g_tex, touched = np.stack([p[0] for p in parts]), np.stack([p[4] for p in parts])
    if not per_view:
        g_tex, touched = g_tex[:1] + g_tex[1:], touched[:1] | touched[1:]
    return (g_tex,) + tuple(np.stack([p[k] for p in parts]) for k in (1, 2, 3)) + (touched,)


@pytest.mark.parametrize("per_view", [True, False])
@pytest.mark.parametrize("with_bias", [False, True])
def test_trilinear_lookup(per_view, with_bias):
    from gaussianip_amd.utils.rasterize import DiffMeshRasterizerContext
    c = _lookup_inputs("spread")
    level = _levels_of(c, with_bias)
    assert (level < 0).sum() > 20 and (level > c["L"]).sum() > 20 and ((level > 0) & (level < c["L"])).sum() > 60
    ctx = _ctx()
    tex = _cu(c["tex"] if per_view else c["tex"][0])
    uv, uv_da, bias = _cu(c["uv"]), _cu(c["uv_da"]), (_cu(c["bias"]) if with_bias else None)
    before = _counts()
    out = ctx.texture(tex, uv, uv_da=uv_da, mip_level_bias=bias)        # "auto": linear-mipmap-linear
    assert _launches(before) == {"gip_mesh_mip_levels": 1, "gip_mesh_mip_build": 1, "gip_mesh_texture_mip": 1}
    assert out.shape == PIX + (TC,)
    tag = "%s_%s" % ("per_view" if per_view else "shared", "bias" if with_bias else "nobias")
    _rule("trilinear_" + tag, _np(out), _want(c, per_view, with_bias, F64), _want(c, per_view, with_bias, F32))
    assert torch.equal(out, ctx.texture(tex, uv, filter_mode="linear-mipmap-linear", uv_da=uv_da, mip_level_bias=bias))
    # where the level is clamped to 0, the parent's bilinear lookup bit for bit
    plain = DiffMeshRasterizerContext().texture(tex, uv)
    assert torch.equal(plain, ctx.texture(tex, uv)) and torch.equal(plain, ctx.texture(tex, uv, filter_mode="linear"))
    at0 = torch.from_numpy(level <= 0).cuda()
    assert torch.equal(out[at0], plain[at0]) and not torch.equal(out[~at0], plain[~at0])
    # a prebuilt stack: the same tensor, and no build
    stack = ctx.texture_construct_mip(tex)
    before = _counts()
    again = ctx.texture(tex, uv, uv_da=uv_da, mip_level_bias=bias, mip=stack)
    assert _launches(before) == {"gip_mesh_texture_mip": 1} and torch.equal(again, out)
    if with_bias and per_view:      # the bias alone sets the level
        only = ctx.texture(tex, uv, mip_level_bias=bias)
        _levels_of(c, True, with_da=False)
        _rule("trilinear_bias_only", _np(only), _want(c, True, True, F64, with_da=False), _want(c, True, True, F32, with_da=False))
        capped = ctx.texture(tex, uv, uv_da=uv_da, mip_level_bias=bias, max_mip_level=0)      # L = 0: bilinear everywhere
        assert torch.equal(capped, plain)


def test_a_texture_without_levels_is_the_bilinear_lookup():
    from gaussianip_amd.utils.rasterize import DiffMeshRasterizerContext
    c = _lookup_inputs("spread")
    tex = _cu(np.random.default_rng(33).uniform(0, 1, (7, 7, 3)).astype(np.float32))      # odd sides: L = 0
    ctx = _ctx()
    uv, uv_da = _cu(c["uv"]), _cu(c["uv_da"])
    before = _counts()
    out = ctx.texture(tex, uv, uv_da=uv_da, mip_level_bias=_cu(c["bias"]))
    assert _launches(before) == {"gip_mesh_mip_levels": 1, "gip_mesh_texture_mip": 1}
    assert torch.equal(out, DiffMeshRasterizerContext().texture(tex, uv))


# ---------------------------------------------------------------------------------------------------------------- 5. gradients
@pytest.mark.parametrize("kind,per_view", [("spread", True), ("spread", False), ("corner", False)])
def test_gradients_of_the_trilinear_lookup(kind, per_view):
    c = _lookup_inputs(kind)
    L = c["L"]
    level = _levels_of(c, True)
    g = np.random.default_rng(40).normal(size=PIX + (TC,)).astype(np.float32)
    ctx = _ctx()
    tex = _cu(c["tex"] if per_view else c["tex"][0]).requires_grad_(True)
    uv, uv_da, bias = (_cu(c[k]).requires_grad_(True) for k in ("uv", "uv_da", "bias"))
    before = _counts()
    out = ctx.texture(tex, uv, uv_da=uv_da, mip_level_bias=bias)
    (out * _cu(g)).sum().backward()
    assert _launches(before) == {"gip_mesh_mip_levels": 1, "gip_mesh_mip_build": 1, "gip_mesh_texture_mip": 1,
                                 "gip_mesh_texture_mip_backward": 1, "gip_mesh_mip_fold": 1}
    w64, w32 = _want_grad(c, per_view, True, g, F64), _want_grad(c, per_view, True, g, F32)
    tag = "%s_%s" % (kind, "per_view" if per_view else "shared")
    got_tex = _np(tex.grad).reshape(w64[0].shape)
    bar_tex = _rule("grad_trilinear_tex_" + tag, got_tex, w64[0], w32[0])
    _rule("grad_trilinear_uv_" + tag, _np(uv.grad), w64[1], w32[1])
    _rule("grad_trilinear_uv_da_" + tag, _np(uv_da.grad), w64[2], w32[2])
    _rule("grad_trilinear_bias_" + tag, _np(bias.grad), w64[3], w32[3])
    touched = w64[4] | w32[4]
    assert not got_tex[~touched].any()                                 # exactly 0 where no footprint's block reaches
    if kind == "corner":
        assert (~touched).sum() > 20 and level.max() < 2.5
    clamped = (level <= 0) | (level >= L)
    assert not _np(uv_da.grad)[clamped].any() and not _np(bias.grad)[clamped].any()
    if kind == "spread":
        assert clamped.sum() > 40 and (~clamped).sum() > 60
        assert np.abs(_np(bias.grad)[~clamped]).min() > 0
    # with a prebuilt stack the gradient still reaches tex
    stack = ctx.texture_construct_mip(tex)
    first = tex.grad.clone()
    tex.grad = None
    (ctx.texture(tex, uv.detach(), uv_da=uv_da.detach(), mip_level_bias=bias.detach(), mip=stack) * _cu(g)).sum().backward()
    assert float((tex.grad - first).abs().max()) <= bar_tex * float(np.abs(w64[0]).max())
    # Linearity in the texture, as tests/test_gpu_mesh_render.py checks it for the fused shade: <p, lookup(tex)> - <p, lookup(0)> =
    # <dL/dtex, tex> with a positive upstream gradient p and a positive texture (terms of one sign), to the sum of the two bars.
    p = np.random.default_rng(41).uniform(0.5, 1.5, size=PIX + (TC,)).astype(np.float32)
    tex.grad = None
    lit = ctx.texture(tex, uv.detach(), uv_da=uv_da.detach(), mip_level_bias=bias.detach())
    (lit * _cu(p)).sum().backward()
    with torch.no_grad():
        dark = ctx.texture(torch.zeros_like(tex), uv.detach(), uv_da=uv_da.detach(), mip_level_bias=bias.detach())
    lhs = float((p.astype(F64) * (_np(lit).astype(F64) - _np(dark).astype(F64))).sum())
    rhs = float((_np(tex.grad).astype(F64) * (c["tex"] if per_view else c["tex"][0])).sum())
    o64, o32 = _want(c, per_view, True, F64), _want(c, per_view, True, F32)
    bar = FACTOR * float(np.abs(o32 - o64).max() / np.abs(o64).max()) + FLOOR + bar_tex
    err = abs(lhs - rhs) / abs(lhs)
    print("linearity %s: %.9g vs %.9g, relative difference %.3e, bar %.3e" % (tag, lhs, rhs, err, bar))
    _figures["linearity_" + tag] = dict(lhs=lhs, rhs=rhs, relative_difference=err, bar=bar)
    assert err <= bar


# ---------------------------------------------------------------------------------------------------------------- 6. mipmap-nearest
def test_linear_mipmap_nearest():
    c = _lookup_inputs("spread")
    _levels_of(c, True)
    g = np.random.default_rng(50).normal(size=PIX + (TC,)).astype(np.float32)
    ctx = _ctx()
    tex = _cu(c["tex"]).requires_grad_(True)
    uv, uv_da, bias = (_cu(c[k]).requires_grad_(True) for k in ("uv", "uv_da", "bias"))
    out = ctx.texture(tex, uv, filter_mode="linear-mipmap-nearest", uv_da=uv_da, mip_level_bias=bias)
    _rule("nearest", _np(out), _want(c, True, True, F64, nearest=True), _want(c, True, True, F32, nearest=True))
    trilinear = _want(c, True, True, F64)
    assert np.abs(trilinear - _want(c, True, True, F64, nearest=True)).max() > 0.05      # not the same lookup
    (out * _cu(g)).sum().backward()
    w64, w32 = _want_grad(c, True, True, g, F64, nearest=True), _want_grad(c, True, True, g, F32, nearest=True)
    _rule("grad_nearest_tex", _np(tex.grad), w64[0], w32[0])
    _rule("grad_nearest_uv", _np(uv.grad), w64[1], w32[1])
    assert not _np(uv_da.grad).any() and not _np(bias.grad).any()      # the level is piecewise constant
    assert not _np(tex.grad)[~(w64[4] | w32[4])].any()


# ---------------------------------------------------------------------------------------------------------------- 7. the chain
T_CHECK = 64
EDGE = 1e-4                    # pixels whose float64 level lies this close to an integer or a clamp may be left out
LEFT_OUT_CAP = 0.005           # of the covered pixels, at most


@functools.lru_cache(maxsize=None)
def _chain():
    """rasterize -> interpolate(uv, rast, tri, rast_db, "all") -> texture on the perspective grid, restated in both precisions.  Every
    vertex has a random s in (0.05, 0.95): a triangle of about 8 pixels spans some 20 texels of the 64 x 64 checkerboard along s.

    With checks of one texel, a bilinear lookup is 0.5 + (c - 0.5) (1 - 2 fx) (1 - 2 fy) with c the 0 or 1 of its first texel, so at
    sub-texel phases (fx, fy) spread evenly, which is what any smooth map gives once it minifies, its standard deviation is 0.5 / 3 =
    0.167 however strongly the scene minifies.  To show the aliasing at full strength along s, every vertex has its t within a tenth
    of a texel of the centre of texel row 31: fy stays near 0 and the standard deviation is 0.5 / sqrt(3) = 0.29."""
    s = _scene("grid")
    rng = np.random.default_rng(70)
    V = s["pos"].shape[1]
    attr = np.stack((rng.uniform(0.05, 0.95, V), (31.5 + rng.uniform(-0.1, 0.1, V)) / T_CHECK), 1).astype(np.float32)
    yy, xx = np.mgrid[0:T_CHECK, 0:T_CHECK]
    tex = ((yy + xx) % 2).astype(np.float32)[..., None]                # checks of one texel: every level >= 1 is exactly 0.5
    out = {}
    for dt, b, db in ((F64, s["b64"], s["db64"]), (F32, s["b32"], s["db32"])):
        st = ref.interpolate(attr, s["tri"], s["ids"], b[0], b[1], dt)
        st_da = mref.interpolate_da(attr, s["tri"], s["ids"], db, None, dt)
        levels = mref.mip_build(tex, None, dt)
        assert all((t == 0.5).all() for t in levels[1:])
        out[dt] = dict(st=st, st_da=st_da, level=mref.lod(st_da, None, T_CHECK, T_CHECK, st.shape[:-1], dt)["level"],
                       value=np.stack([mref.texture_mip(levels, st[v], st_da[v], None, dt) for v in range(st.shape[0])]))
    level = out[F64]["level"]
    L = mref.mip_levels(T_CHECK, T_CHECK)
    with np.errstate(invalid="ignore"):
        keep = (np.abs(level - np.rint(level)) > EDGE) | (level < -EDGE) | (level > L + EDGE)
    keep &= np.isfinite(level)
    return dict(attr=attr, tex=tex, keep=keep, level=level, **{("w64" if dt is F64 else "w32"): out[dt]["value"] for dt in out},
                st64=out[F64]["st"])


def test_the_chain_on_the_perspective_grid():
    from gaussianip_amd.utils.rasterize import DiffMeshRasterizerContext
    s, c = _scene("grid"), _chain()
    keep, level = c["keep"], c["level"]
    covered = int((s["ids"] >= 0).sum())
    assert (~keep).sum() <= LEFT_OUT_CAP * covered, ((~keep).sum(), covered)
    ctx = _ctx()
    rast, db = ctx.rasterize(_cu(s["pos"]), _cu(s["tri"]), (H, W))
    st, st_da = ctx.interpolate(_cu(c["attr"]), rast, _cu(s["tri"]), rast_db=db, diff_attrs="all")
    tex = _cu(c["tex"])
    out = ctx.texture(tex, st, uv_da=st_da)
    assert out.shape == (2, H, W, 1)
    _rule("chain", _np(out)[keep], c["w64"][keep], c["w32"][keep])
    minified = keep & (level >= 1)
    assert minified.sum() >= 200
    assert np.abs(_np(out)[minified] - 0.5).max() <= 1e-6
    plain = _np(DiffMeshRasterizerContext().texture(tex, st))
    print("chain: %d pixels at level >= 1 of %d, %d left out; the bilinear lookup there has a standard deviation of %.3f" % (
        minified.sum(), covered, (~keep).sum(), plain[minified].std()))
    _figures["chain_minified"] = dict(pixels=int(minified.sum()), left_out=int((~keep).sum()), bilinear_std=float(plain[minified].std()))
    assert plain[minified].std() > 0.2                                 # the scene really minifies there: bilinear aliases


# ---------------------------------------------------------------------------------------------------------------- 8. arguments
def test_argument_errors_and_no_faces():
    s = _scene("grid")
    ctx = _ctx()
    p, t = _cu(s["pos"]), _cu(s["tri"])
    rast, db = ctx.rasterize(p, t, (H, W))
    attr = torch.zeros((s["pos"].shape[1], 5), device="cuda")
    for kw in (dict(rast_db=db), dict(diff_attrs="all")):              # one without the other
        with pytest.raises(ValueError, match="go together"):
            ctx.interpolate(attr, rast, t, **kw)
    for bad in ([5], [-1], [0, 7], [], "some"):
        with pytest.raises(ValueError, match="diff_attrs"):
            ctx.interpolate(attr, rast, t, rast_db=db, diff_attrs=bad)
    for bad in (db[:1], db[..., :3], db.cpu(), db.double(), db[:, :10]):
        with pytest.raises(ValueError, match="rast_db"):
            ctx.interpolate(attr, rast, t, rast_db=bad, diff_attrs="all")
    with pytest.raises(ValueError):
        ctx.interpolate(attr.cpu(), rast, t, rast_db=db, diff_attrs="all")
    tex, uv = torch.rand((16, 8, 3), device="cuda"), torch.rand((2, 4, 5, 2), device="cuda")
    uv_da, bias = torch.rand((2, 4, 5, 4), device="cuda"), torch.zeros((2, 4, 5), device="cuda")
    with pytest.raises(NotImplementedError, match="filter_mode"):
        ctx.texture(tex, uv, filter_mode="nearest")
    with pytest.raises(NotImplementedError, match="filter_mode"):
        ctx.texture(tex, uv, filter_mode="cubic")
    for mode in ("wrap", "zero", "cube"):
        with pytest.raises(NotImplementedError, match="boundary_mode"):
            ctx.texture(tex, uv, uv_da=uv_da, boundary_mode=mode)
    with pytest.raises(NotImplementedError, match="mip"):
        ctx.texture(tex, uv, uv_da=uv_da, mip=[tex[None], tex[None, ::2, ::2]])
    other = ctx.texture_construct_mip(torch.rand((8, 8, 3), device="cuda"))
    with pytest.raises(ValueError, match="mip"):
        ctx.texture(tex, uv, uv_da=uv_da, mip=other)                   # built from a texture of another shape
    with pytest.raises(ValueError, match="mip"):
        ctx.texture(tex, uv, uv_da=uv_da, mip="stack")
    with pytest.raises(ValueError, match="max_mip_level"):
        ctx.texture(tex, uv, uv_da=uv_da, mip=ctx.texture_construct_mip(tex), max_mip_level=1)
    with pytest.raises(ValueError, match="max_mip_level"):
        ctx.texture_construct_mip(tex, max_mip_level=-2)
    for bad_kw in (dict(uv_da=uv_da[..., :3]), dict(uv_da=uv_da[:1]), dict(uv_da=uv_da.cpu()), dict(uv_da=uv_da.double()),
                   dict(mip_level_bias=bias[..., None]), dict(mip_level_bias=bias.cpu()), dict(uv_da=uv_da, filter_mode="linear")):
        with pytest.raises(ValueError):
            ctx.texture(tex, uv, **bad_kw)
    for bad_tex, bad_uv in ((tex.cpu(), uv), (tex.double(), uv), (tex[0], uv), (tex, uv[..., :1]), (tex, uv.cpu()),
                            (torch.zeros((3, 4, 4, 3), device="cuda"), uv)):
        with pytest.raises(ValueError):
            ctx.texture(bad_tex, bad_uv, uv_da=uv_da)
    with pytest.raises(ValueError):
        ctx.texture_construct_mip(tex.cpu())
    # F == 0 launches nothing and returns zeros
    none = torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    before = _counts()
    rast0, db0 = ctx.rasterize(torch.zeros((2, 4, 4), device="cuda"), none, (H, W))
    assert _launches(before) == {} and rast0.shape == db0.shape == (2, H, W, 4) and not rast0.any() and not db0.any()
    one_rast, one_db = ctx.rasterize_one(torch.zeros((4, 4), device="cuda"), none, 8)
    assert one_rast.shape == one_db.shape == (8, 8, 4) and not one_db.any()
