"""Rendered views projected onto the texture atlas, on the GPU (csrc/texture_project.hip, utils.texture.visible_depth / project_views,
GaussianModel.bake_texture_from_views, extract_textured_mesh(bake="views")).

Float64 side: tests/texture_project_reference.py, the definition restated in numpy.  Bar, the rule of tests/test_gpu_texture.py: errors
normalised by the output's maximum, at most 4 times the float32 error of the restatement against itself in float64 plus a floor of
2e-6.  It is taken over the texels that the restatement does not flag as "some decision of some view could flip" (at most 2 % of the
owned texels in every case: tests/test_texture_project_cpu.py holds the restatement to that cap on its own); on those the count of
views must be equal exactly.

With GIP_TEXTURE_PROJECT_PARITY_OUT=<file> the figures are written there as JSON (profiles/texture_project_parity.json is such a run)."""
import functools
import json
import math
import os
import types
from argparse import ArgumentParser

import numpy as np
import pytest
import torch

import mesh_render_inputs
import mesh_render_reference as mref
import sample_inputs
import scenes
import texture_project_inputs as inputs
import texture_project_reference as ref

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 4.0, 2e-6
_figures = {}


@pytest.fixture(scope="module", autouse=True)
def _write_figures():
    yield
    out = os.environ.get("GIP_TEXTURE_PROJECT_PARITY_OUT")
    if out and _figures:
        with open(out, "w") as f:
            json.dump(_figures, f, indent=1, sort_keys=True)


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _calls():
    from gaussianip_amd import _lib
    return _lib.call_counts.get("gip_texture_project", 0)


def _cams(projs, centres, h, w):
    """What visible_depth and project_views read of a camera."""
    return [types.SimpleNamespace(full_proj_transform=_cu(np.asarray(m, np.float32)), camera_center=_cu(np.asarray(c, np.float32)), image_height=h,
                                  image_width=w) for m, c in zip(projs, centres)]


def _run(sc, two_sided=True, unpremultiply=False, launches=1, **kw):
    """One project_views of a scene of the inputs module, with the count of calls of the HIP entry point checked."""
    from gaussianip_amd.utils import texture as tex
    images = _cu(sc["images"][..., :3].transpose(0, 3, 1, 2))
    alphas = _cu(sc["images"][..., 3:].transpose(0, 3, 1, 2))
    before = _calls()
    out = tex.project_views(_cu(sc["vertices"]), _cu(sc["faces"]), sc["T"], _cams(sc["projs"], sc["centres"], sc["H"], sc["W"]), images,
                            _cu(sc["vis_depth"]), depth_tolerance=sc["depth_tolerance"], alphas=alphas, two_sided=two_sided,
                            unpremultiply=unpremultiply, **kw)
    assert _calls() == before + launches
    T, F = sc["T"], len(sc["faces"])
    assert set(out) == {"color_sum", "weight_sum", "count", "uv", "cell"}
    assert out["color_sum"].shape == (T, T, 3) and out["weight_sum"].shape == (T, T) and out["count"].shape == (T, T) and out["uv"].shape == (F, 3, 2)
    assert out["color_sum"].dtype == torch.float32 and out["weight_sum"].dtype == torch.float32 and out["count"].dtype == torch.int32
    return out


def _restated(sc, two_sided=True, unpremultiply=False, **kw):
    args = (sc["vertices"], sc["faces"], sc["T"], sc["views"], sc["images"], sc["vis_depth"], sc["depth_tolerance"])
    return tuple(ref.project(*args, two_sided=two_sided, unpremultiply=unpremultiply, dtype=dt, **kw) for dt in (np.float64, np.float32))


def _against_float64(name, out, f64, f32):
    """The rule of the module's docstring for the two sums; counts equal on unflagged texels; unowned texels exactly 0."""
    owned, flagged = f64["owned"], f64["flagged"]
    sure = owned & ~flagged
    share = flagged.sum() / max(owned.sum(), 1)
    assert share <= inputs.FLAG_CAP, (name, share)
    count = _np(out["count"])
    assert not count[~owned].any() and not _np(out["color_sum"])[~owned].any() and not _np(out["weight_sum"])[~owned].any(), name
    differ = int((count[sure] != f64["count"][sure]).sum())
    print("%s: %d owned texels, %d flagged, %d counts differ among the unflagged" % (name, owned.sum(), flagged.sum(), differ))
    figures = dict(owned=int(owned.sum()), flagged=int(flagged.sum()), counts_differ=differ)
    worst = []
    for key in ("color_sum", "weight_sum"):
        got = _np(out[key]).astype(np.float64)
        assert np.isfinite(got).all(), (name, key)
        mx = np.abs(f64[key]).max()
        if mx == 0:
            assert not got.any()
            continue
        ref_err = float(np.abs(f32[key].astype(np.float64) - f64[key])[sure].max() / mx)
        err = float(np.abs(got - f64[key])[sure].max() / mx)
        bar = FACTOR * ref_err + FLOOR
        print("%s %s: kernel %.3e reference %.3e bar %.3e" % (name, key, err, ref_err, bar))
        figures[key] = dict(kernel_err=err, reference_err=ref_err, bar=bar)
        worst.append((key, err, bar))
    _figures[name] = figures
    assert differ == 0, name
    for key, err, bar in worst:
        assert err <= bar, (name, key, err, bar)


# ---------------------------------------------------------------------------------------------------------------- 1. parity
@functools.lru_cache(maxsize=None)
def _parity(two_sided, unpremultiply):
    return _restated(inputs.parity_scene(), two_sided, unpremultiply)


def test_parity_scene_contents():
    """The parity scene holds every case the kernel distinguishes; asserted from the restatement (the CPU suite asserts the same)."""
    import test_texture_project_cpu as cpu
    sc = inputs.parity_scene()
    f64, _ = _parity(True, False)
    assert f64["owned"].sum() == 2880 and sc["K"] == 3 and (sc["H"], sc["W"]) == (45, 67) and sc["T"] == 64
    found, seen = cpu.parity_scene_content(f64, sc)
    assert all(found.values()), found
    assert len(seen) == 4 and (seen > 0).all(), seen


@pytest.mark.parametrize("two_sided,unpremultiply", inputs.FLAG_COMBINATIONS)
def test_parity_against_float64(two_sided, unpremultiply):
    sc = inputs.parity_scene()
    f64, f32 = _parity(two_sided, unpremultiply)
    out = _run(sc, two_sided, unpremultiply)
    assert out["cell"] == 12
    _against_float64("parity_two_sided%d_unpremultiply%d" % (two_sided, unpremultiply), out, f64, f32)
    # the degenerate face contributes nothing
    run = f64["run64"]
    dead = ~run["live"]
    assert dead.any() and not _np(out["count"])[run["y"][dead], run["x"][dead]].any()


# ---------------------------------------------------------------------------------------------------------------- 2. extremes
@pytest.mark.parametrize("name", inputs.EXTREMES)
def test_layout_extremes(name):
    sc = inputs.extreme_scene(name)
    F, T, K = (int(s[1:]) for s in name.split("_"))
    assert len(sc["faces"]) == F and sc["T"] == T and sc["K"] == K
    f64, f32 = _restated(sc)
    c = ref.texture_reference.layout(F, T)[0]
    if name == "F128_T32_K64":
        assert c == 4 and f64["owned"].all() and (sc["H"], sc["W"]) == (12, 16)      # the atlas is full
    if name == "F7_T21_K3":
        assert T & (T - 1) and not f64["owned"].all()
    out = _run(sc)
    assert out["cell"] == c and int(out["count"].max()) >= 1
    _against_float64("extreme_" + name, out, f64, f32)


@pytest.mark.parametrize("K", [0, 65])
def test_view_count_out_of_range(K):
    from gaussianip_amd.utils import texture as tex
    sc = inputs.extreme_scene("F2_T16_K3")
    cams = (_cams(sc["projs"], sc["centres"], sc["H"], sc["W"]) * 22)[:K]
    images = torch.zeros((K, 3, sc["H"], sc["W"]), device="cuda")
    vis = torch.zeros((K, sc["H"], sc["W"]), device="cuda")
    before = _calls()
    with pytest.raises(ValueError, match="1 .. 64"):
        tex.project_views(_cu(sc["vertices"]), _cu(sc["faces"]), sc["T"], cams, images, vis, depth_tolerance=0.05)
    assert _calls() == before


def test_argument_errors():
    from gaussianip_amd.utils import texture as tex
    sc = inputs.extreme_scene("F2_T16_K3")
    v, f = _cu(sc["vertices"]), _cu(sc["faces"])
    cams = _cams(sc["projs"], sc["centres"], sc["H"], sc["W"])
    images, vis = torch.zeros((3, 3, sc["H"], sc["W"]), device="cuda"), torch.zeros((3, sc["H"], sc["W"]), device="cuda")
    kw = dict(depth_tolerance=0.05)
    before = _calls()
    with pytest.raises(ValueError):
        tex.project_views(v, f.long(), 16, cams, images, vis, **kw)                 # not int32
    with pytest.raises(ValueError):
        tex.project_views(v[:, :2], f, 16, cams, images, vis, **kw)
    with pytest.raises(ValueError, match="images"):
        tex.project_views(v, f, 16, cams, images[:2], vis, **kw)
    with pytest.raises(ValueError, match="images"):
        tex.project_views(v, f, 16, cams, images.double(), vis, **kw)
    with pytest.raises(ValueError, match="vis_depth"):
        tex.project_views(v, f, 16, cams, images, vis[:, :-1], **kw)
    with pytest.raises(ValueError, match="alphas"):
        tex.project_views(v, f, 16, cams, images, vis, alphas=images, **kw)
    with pytest.raises(ValueError, match="min_alpha"):
        tex.project_views(v, f, 16, cams, images, vis, unpremultiply=True, min_alpha=0.0, **kw)
    with pytest.raises(ValueError, match="texture_size"):
        tex.project_views(v, f, 3, cams, images, vis, **kw)
    with pytest.raises(ValueError, match="smallest size"):                          # 40 faces need 5 cells per row: 20 texels
        tex.project_views(v.repeat(20, 1), f.repeat(20, 1), 16, cams, images, vis, **kw)
    bad = f.clone()
    bad[1, 2] = v.shape[0]
    with pytest.raises(ValueError, match="indices"):
        tex.project_views(v, bad, 16, cams, images, vis, **kw)
    bad[1, 2] = -1
    with pytest.raises(ValueError, match="indices"):
        tex.project_views(v, bad, 16, cams, images, vis, **kw)
    assert _calls() == before
    none = tex.project_views(v, f[:0], 16, cams, images, vis, **kw)                    # no faces: zeros, no launch
    assert _calls() == before and not none["count"].any() and none["uv"].shape == (0, 3, 2)


# ---------------------------------------------------------------------------------------------------------------- 3. determinism
def test_determinism_and_an_invisible_view():
    sc = inputs.parity_scene()
    a, b = _run(sc), _run(sc)
    for key in ("color_sum", "weight_sum", "count"):
        assert torch.equal(a[key], b[key]), key
    assert int(a["count"].max()) == 3
    # one more view whose alpha is 0 everywhere: nothing changes, bit for bit
    more = dict(sc)
    more["images"] = np.concatenate((sc["images"], sc["images"][1:2] * np.array([1, 1, 1, 0], np.float32)))
    for key in ("projs", "centres", "vis_depth"):
        more[key] = np.concatenate((sc[key], sc[key][1:2]))
    more["K"] = 4
    c = _run(more)
    for key in ("color_sum", "weight_sum", "count"):
        assert torch.equal(a[key], c[key]), key


def test_a_constant_image_gives_its_colour():
    sc = dict(inputs.extreme_scene("F1_T16_K1"))
    col = np.array([0.3, 0.9, 0.6], np.float32)
    sc["images"] = np.broadcast_to(np.append(col, np.float32(1)), sc["images"].shape).astype(np.float32).copy()
    f64, f32 = _restated(sc)
    out = _run(sc)
    _against_float64("constant_image", out, f64, f32)
    assert int(out["count"].sum()) > 0
    # color_sum = weight_sum * the constant, to the same rule (the reference error: the restatement's own on this identity)
    want = _np(out["weight_sum"]).astype(np.float64)[..., None] * col.astype(np.float64)
    mx = np.abs(f64["color_sum"]).max()
    ref_err = float(np.abs(f32["color_sum"].astype(np.float64) - f64["weight_sum"][..., None] * col.astype(np.float64)).max() / mx)
    err = float(np.abs(_np(out["color_sum"]).astype(np.float64) - want).max() / mx)
    bar = FACTOR * ref_err + FLOOR
    print("constant image: color_sum - weight_sum * colour %.3e, reference %.3e, bar %.3e" % (err, ref_err, bar))
    _figures["constant_image_identity"] = dict(kernel_err=err, reference_err=ref_err, bar=bar)
    assert err <= bar


# ---------------------------------------------------------------------------------------------------------------- 4. round trip
def test_round_trip_through_the_rasterizer():
    """A linear ramp in pixel coordinates projected onto a fronto-parallel mesh and rendered back from the same camera reproduces
    itself: visible_depth -> project_views -> normalise -> render_mesh.  The reference is the same chain restated
    (texture_project_reference, then mesh_render_reference.shade)."""
    from gaussianip_amd.utils import texture as tex
    from gaussianip_amd.utils.rasterize import render_mesh
    H, W = inputs.H, inputs.W
    world, tri = inputs.plane_scene()
    T, tol = inputs.PLANE_SIZE, 0.05
    proj, centre = mesh_render_inputs.EXACT_PROJ, np.zeros(3, np.float32)
    cam = _cams([proj], [centre], H, W)
    pos = mesh_render_inputs.exact_clip(world)[None]                  # the positions visible_depth rasterizes, bit for bit
    ids = mref.rasterize(pos, tri, H, W)["tri"]
    assert (ids >= 0).all()                                            # the grid covers the image
    # visible_depth against the plane's w
    vis = tex.visible_depth(cam, _cu(world), _cu(tri))
    assert vis.shape == (1, H, W) and vis.dtype == torch.float32
    v64, v32 = (ref.visible_depth(pos, tri, H, W, dt) for dt in (np.float64, np.float32))
    assert np.abs(v64 - inputs.PLANE_W).max() < 1e-12
    ref_err = float(np.abs(v32.astype(np.float64) - v64).max() / inputs.PLANE_W)
    err = float(np.abs(_np(vis).astype(np.float64) - inputs.PLANE_W).max() / inputs.PLANE_W)
    bar = FACTOR * ref_err + FLOOR
    print("visible_depth on the plane: kernel %.3e reference %.3e bar %.3e" % (err, ref_err, bar))
    _figures["round_trip_visible_depth"] = dict(kernel_err=err, reference_err=ref_err, bar=bar)
    assert err <= bar
    # the projection
    ramp = inputs.ramp_image()
    image = _cu(ramp[..., :3].transpose(2, 0, 1)[None])
    out = tex.project_views(_cu(world), _cu(tri), T, cam, image, vis, depth_tolerance=tol, min_alpha=0.0)
    texture = torch.where((out["count"] > 0).unsqueeze(2), out["color_sum"] / out["weight_sum"].clamp_min(1e-30).unsqueeze(2),
                          torch.zeros_like(out["color_sum"]))
    rendered = render_mesh(cam[0], _cu(world), _cu(tri), out["uv"], texture)
    got = _np(rendered["image"]).transpose(1, 2, 0).astype(np.float64)
    # the restated chain
    views = ref.pack_views([proj], [centre])
    uv = _np(out["uv"])
    flipped = np.stack((uv[..., 0], np.float32(1) - uv[..., 1]), -1)
    chain, flagged = {}, None
    for dt in (np.float64, np.float32):
        r = ref.project(world, tri, T, views, ramp[None], v32, tol, min_alpha=0.0, dtype=dt)
        with np.errstate(all="ignore"):
            t = np.where((r["count"] > 0)[..., None], r["color_sum"] / r["weight_sum"][..., None], dt(0)).astype(dt)
        u, v, _ = mref.barycentrics(pos, tri, H, W, ids, dt)
        chain[dt] = mref.shade(t, flipped, ids, u, v, np.zeros(3), dt)[0][0]
        if dt is np.float64:
            flagged = r["flagged"]
            assert flagged.sum() <= inputs.FLAG_CAP * r["owned"].sum()
            st = mref.interpolate(flipped.reshape(-1, 2), np.arange(len(tri) * 3).reshape(-1, 3), ids, u, v, dt)[0]
            x0, x1, y0, y1, _, _ = mref.lookup_setup(st, T, T, dt)
            touched = flagged[y0, x0] | flagged[y0, x1] | flagged[y1, x0] | flagged[y1, x1]
    # covered pixels whose four neighbours are covered (and whose footprint holds no flagged texel)
    covered = _np(rendered["alpha"])[0] > 0
    assert covered.all()
    inner = np.zeros((H, W), bool)
    inner[1:-1, 1:-1] = covered[1:-1, 1:-1] & covered[:-2, 1:-1] & covered[2:, 1:-1] & covered[1:-1, :-2] & covered[1:-1, 2:]
    inner &= ~touched
    assert inner.sum() >= (H - 2) * (W - 2) * 0.95
    want = ramp[..., :3].astype(np.float64)
    mx = np.abs(want).max()
    ref_err = float(np.abs(chain[np.float32].astype(np.float64) - chain[np.float64])[inner].max() / mx)
    chain_err = float(np.abs(chain[np.float64] - want)[inner].max() / mx)
    err = float(np.abs(got - want)[inner].max() / mx)
    err_chain = float(np.abs(got - chain[np.float64])[inner].max() / mx)
    bar = FACTOR * ref_err + FLOOR
    print("round trip over %d pixels: render - ramp %.3e, render - restated chain %.3e, float64 chain - ramp %.3e, reference %.3e, bar %.3e" %
          (inner.sum(), err, err_chain, chain_err, ref_err, bar))
    _figures["round_trip_ramp"] = dict(kernel_err=err, kernel_vs_chain=err_chain, chain64_vs_ramp=chain_err, reference_err=ref_err, bar=bar,
                                       pixels=int(inner.sum()))
    assert err <= bar and err_chain <= bar


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
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


def _camera(el, az, dist, target, fovy_deg, size):
    """A camera of the project on the orbit of scenes.orbit_c2w, moved so that `target` lands on the image centre at depth `dist`
    (tests/test_gpu_mesh_render.py explains the move)."""
    from gaussianip_amd.scene import Camera
    c2w = scenes.orbit_c2w(el, az, dist)
    rot = c2w[:3, :3].clone()
    c2w[:3, 3] -= rot @ torch.diag(torch.tensor([1.0, -1.0, -1.0])) @ rot.t() @ torch.tensor(target, dtype=torch.float32)
    return Camera(c2w=c2w.cuda(), FoVy=math.radians(fovy_deg), height=size, width=size)


AXES = [(0.0, 0.0), (0.0, 90.0), (0.0, 180.0), (0.0, 270.0), (89.0, 0.0), (-89.0, 0.0)]      # the poles: 89 degrees, where the orbit's up is defined


def test_one_gaussian_end_to_end():
    """The sphere of one isotropic Gaussian, every Gaussian of the cloud given the colour `col`, rendered over a background of `col`:
    the six images are constant, so every texel that a view passes is `col`, and with six cameras along the axes every texel of a
    face that has a normal is passed by one (the best camera sees a face at cos >= 1 / sqrt(3))."""
    from gaussianip_amd import _lib
    from gaussianip_amd.arguments import PipelineParams
    from gaussianip_amd.renderer import render_views
    from gaussianip_amd.utils import texture as tex
    cl, _ = sample_inputs.sphere_cloud()
    col = np.array(sample_inputs.SPHERE_COLOR, np.float32)
    gm = _model(cl, np.tile(col, (cl["xyz"].shape[0], 1)))
    pipe = PipelineParams(ArgumentParser())
    size = 96
    cams = [_camera(el, az, 3.0, sample_inputs.SPHERE_MU, 20.0, size) for el, az in AXES]
    with torch.no_grad():
        pkg = render_views(cams, gm, pipe, _cu(col))
    images = pkg["render"].detach().contiguous()
    assert float((images - _cu(col)[None, :, None, None]).abs().max()) <= 1e-6      # constant, to rounding
    kw = dict(density_thresh=sample_inputs.SPHERE_THRESHOLD, resolution=32, num_blocks=4)
    view_kw = dict(images=images, min_alpha=0.0, unpremultiply=False)
    before = _calls()
    v, f, n, uv, texture = gm.extract_textured_mesh(bake="views", cameras=cams, pipe=pipe, **kw, **view_kw)
    assert _calls() == before + 1
    v0, f0, n0, uv0, field_texture = gm.extract_textured_mesh(**kw)
    assert _calls() == before + 1                                     # the default path never calls the projection
    assert torch.equal(v, v0) and torch.equal(f, f0) and torch.equal(n, n0) and torch.equal(uv, uv0) and f.shape[0] > 100
    # the default call is bake_texture's path, bit for bit
    field = gm.bake_texture(v, f, None, None, 32, 4, 1.5)
    assert torch.equal(field_texture, field["texture"]) and torch.equal(uv0, field["uv"])
    T = texture.shape[0]
    baked = gm.bake_texture_from_views(v, f, cams, pipe, resolution=32, num_blocks=4, **view_kw)
    assert set(baked) == {"texture", "count", "weight_sum", "uv", "cell"} and torch.equal(baked["texture"], texture)
    # every owned texel of a face with a normal is seen, and is `col`
    owner = tex.texel_owner(f.shape[0], T)
    tri = _np(v)[_np(f).astype(np.int64)]
    normal = np.cross(tri[:, 1].astype(np.float64) - tri[:, 0], tri[:, 2].astype(np.float64) - tri[:, 0])
    has_normal = (normal ** 2).sum(1) > 0
    must = (owner >= 0) & has_normal[np.maximum(owner, 0)]
    count = _np(baked["count"])
    assert (count[must] >= 1).all(), "%d of %d texels unseen" % ((count[must] < 1).sum(), must.sum())
    # the reference error of the rule: the restatement on the images and the visibility that the GPU produced
    vis = tex.visible_depth(cams, v, f)
    tol = 2.0 / 31 / float(gm.scale)
    views = _np(tex.pack_views(cams))
    packed = np.concatenate((_np(images), np.ones((len(cams), 1, size, size), np.float32)), 1).transpose(0, 2, 3, 1)
    tx = {}
    for dt in (np.float64, np.float32):
        r = ref.project(_np(v), _np(f), T, views, packed, _np(vis), tol, min_alpha=0.0, dtype=dt)
        with np.errstate(all="ignore"):
            tx[dt] = np.where((r["count"] > 0)[..., None], r["color_sum"] / r["weight_sum"][..., None], 0).astype(np.float64)
    seen = (count >= 1) & (r["count"] >= 1) & ~r["flagged"]
    mx = float(col.max())
    ref_err = float(np.abs(tx[np.float32] - tx[np.float64])[seen].max() / mx)
    err = float(np.abs(_np(texture).astype(np.float64) - col.astype(np.float64))[count >= 1].max() / mx)
    bar = FACTOR * ref_err + FLOOR
    print("%d faces, texture %d, %d texels seen: colour error %.3e, reference %.3e, bar %.3e" % (f.shape[0], T, (count >= 1).sum(), err, ref_err, bar))
    _figures["sphere_views_colour"] = dict(kernel_err=err, reference_err=ref_err, bar=bar, faces=int(f.shape[0]), texture=int(T))
    assert err <= bar
    # two cameras on one side: the unseen texels are the field bake's, bit for bit
    side = gm.bake_texture_from_views(v, f, cams[:2], pipe, resolution=32, num_blocks=4, images=images[:2], min_alpha=0.0, unpremultiply=False)
    unseen = side["count"] == 0
    owned = _cu(owner >= 0)
    share = float((unseen & owned).sum()) / float(owned.sum())
    print("two cameras: %.3f of the owned texels unseen" % share)
    _figures["sphere_two_cameras_unseen_share"] = share
    assert 0 < share < 1
    assert torch.equal(side["texture"][unseen], field["texture"][unseen])
    assert float((side["texture"][~unseen] - _cu(col)).abs().max()) <= bar * mx
    # rendering the Gaussians inside the method (images=None: black background, unpremultiplied) gives the same colour where it is seen
    inside = gm.bake_texture_from_views(v, f, cams, pipe, resolution=32, num_blocks=4)
    hit = inside["count"] > 0
    assert bool(hit.any()) and float((inside["texture"][hit] - _cu(col)).abs().max()) <= 1e-4
    assert _lib.call_counts.get("gip_texture_project", 0) == before + 4


# ---------------------------------------------------------------------------------------------------------------- 6. recorded only
def test_psnr_against_the_gaussian_render_is_recorded():
    """blob_cloud at 128 x 128 from a camera that is not among the eight baked ones: the PSNR between the Gaussian render and the render
    of the exported mesh, for the field bake and for the bake from views; and the same from one of the eight.  Over the whole image
    the figure is the silhouette's: the iso-surface lies inside the soft edge of the Gaussians.  So it is also taken over the pixels
    that the mesh covers and the Gaussians fill (alpha > 0.9), where it measures the texture.  No bar: it measures the method, not the
    kernel."""
    from gaussianip_amd.arguments import PipelineParams
    from gaussianip_amd.renderer import render
    cl = sample_inputs.blob_cloud()
    gm = _model(cl, sample_inputs.colors(cl["xyz"].shape[0], 9))
    pipe = PipelineParams(ArgumentParser())
    size = 128
    cam = _camera(20.0, 35.0, 2.2, (0.0, 0.0, 0.0), 50.0, size)
    orbit = [_camera(15.0 if i % 2 else -15.0, 45.0 * i, 2.2, (0.0, 0.0, 0.0), 50.0, size) for i in range(8)]
    bg = torch.zeros(3, device="cuda")
    kw = dict(density_thresh=1.0, resolution=64, num_blocks=8)
    psnr = {}
    for where, eye in (("", cam), ("_from_a_baked_camera", orbit[1])):
        with torch.no_grad():
            pkg = render(eye, gm, pipe, bg)
        want, solid = pkg["render"], pkg["alpha_3dgs"][0] > 0.9
        for bake, extra in (("field", {}), ("views", dict(bake="views", cameras=orbit, pipe=pipe))):
            out = gm.render_textured_mesh(eye, bg_color=bg, **kw, **extra)
            both = (out["alpha"][0] > 0) & solid                      # pixels that the mesh covers and the Gaussians fill
            psnr[bake + where] = 10 * math.log10(1 / float(((want - out["image"]) ** 2).mean()))
            psnr[bake + where + "_covered_by_both"] = 10 * math.log10(1 / float(((want - out["image"]) ** 2)[:, both].mean()))
            psnr["pixels_mesh" + where], psnr["pixels_gaussians_alpha_over_half" + where] = int(out["alpha"].sum()), int((pkg["alpha_3dgs"] > 0.5).sum())
    for where in ("", "_from_a_baked_camera"):
        print("blob_cloud, 128 x 128%s: PSNR to the Gaussian render, field bake / bake from 8 views: %.2f / %.2f dB over the image, %.2f / %.2f dB "
              "over the pixels both cover (the mesh covers %d, the Gaussians' alpha is over 0.5 at %d)" % (
                  where.replace("_", " "), psnr["field" + where], psnr["views" + where], psnr["field" + where + "_covered_by_both"],
                  psnr["views" + where + "_covered_by_both"], psnr["pixels_mesh" + where], psnr["pixels_gaussians_alpha_over_half" + where]))
    _figures["blob_cloud_psnr_db"] = psnr
    assert all(math.isfinite(p) for p in psnr.values())
