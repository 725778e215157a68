"""Texture baking on the GPU (csrc/texture.hip, GaussianModel.bake_texture / extract_textured_mesh).

Float64 side: tests/texture_reference.py (the atlas restated from its definition) feeding tests/sample_reference.py.  Bar, errors
normalised by the output's maximum: at most 4 times the float32 error of the restatement against itself in float64 plus a floor of
2e-6 — the rule of tests/test_gpu_field.py; the restatement's error is computed here and printed.

With GIP_TEXTURE_PARITY_OUT=<file> the figures are written there as JSON (profiles/texture_parity.json is such a run)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import field_inputs
import sample_inputs
import texture_inputs
import texture_reference

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 4.0, 2e-6
_figures = {}


@pytest.fixture(scope="module", autouse=True)
def _write_figures():
    yield
    out = os.environ.get("GIP_TEXTURE_PARITY_OUT")
    if out and _figures:
        with open(out, "w") as f:
            json.dump(_figures, f, indent=1, sort_keys=True)


def _model(cl, colors=None):
    from gaussianip_amd.scene import GaussianModel
    from gaussianip_amd.utils.sh import C0
    gm = GaussianModel(0)
    gm._xyz, gm._opacity = torch.from_numpy(cl["xyz"]).cuda(), torch.from_numpy(cl["opacity"]).cuda()
    gm._scaling, gm._rotation = torch.from_numpy(cl["scaling"]).cuda(), torch.from_numpy(cl["rotation"]).cuda()
    P = cl["xyz"].shape[0]
    rgb = np.full((P, 3), 0.5, np.float32) if colors is None else colors
    gm._features_dc = ((torch.from_numpy(rgb).cuda() - 0.5) / C0).reshape(P, 1, 3).contiguous()
    return gm


def _bake(gm, v, f, T, launches=1, **kw):
    """The raw sums of one bake of the normalised mesh (v, f: numpy), with the count of calls of the HIP entry point checked."""
    from gaussianip_amd import _lib
    before = _lib.call_counts.get("gip_texture_bake", 0)
    out = gm._bake_sums(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), T, normalized=True, **kw)
    assert _lib.call_counts.get("gip_texture_bake", 0) == before + launches
    assert out["density"].shape == (T, T) and out["color_sum"].shape == (T, T, 3) and out["uv"].shape == (len(f), 3, 2)
    assert all(out[k].dtype == torch.float32 and out[k].is_cuda for k in ("density", "color_sum", "uv"))
    return out


def _against_float64(name, out, f64, f32):
    """The rule of the module's docstring for density and colour sum; unowned texels exactly 0, everything finite."""
    owned = torch.from_numpy(f64[2]["owned"]).cuda()
    got = {"density": out["density"], "color_sum": out["color_sum"]}
    for i, key in enumerate(("density", "color_sum")):
        g = got[key]
        assert torch.isfinite(g).all() and not g[~owned].any(), key
        mx = np.abs(f64[i]).max()
        ref_err = float(np.abs(f32[i].astype(np.float64) - f64[i]).max() / mx)
        err = float(np.abs(g.cpu().numpy().astype(np.float64) - f64[i]).max() / mx)
        bar = FACTOR * ref_err + FLOOR
        print("%s %s: kernel %.3e reference %.3e bar %.3e" % (name, key, err, ref_err, bar))
        _figures["%s_%s" % (name, key)] = dict(kernel_err=err, reference_err=ref_err, bar=bar)
        assert err <= bar, (name, key, err, ref_err)


# ---------------------------------------------------------------------------------------------------------------- 1. parity
@functools.lru_cache(maxsize=None)
def _scene():
    cl, R, nb = field_inputs.case("b")
    rgb = sample_inputs.colors(cl["xyz"].shape[0], 5)
    v, f, degenerate = texture_inputs.parity_mesh(R, nb)
    T = texture_inputs.PARITY_SIZE
    f64 = texture_reference.bake_sums(cl, rgb, R, nb, v, f, T, np.float64)
    f32 = texture_reference.bake_sums(cl, rgb, R, nb, v, f, T, np.float32)
    return cl, R, nb, rgb, v, f, degenerate, T, f64, f32


def test_parity_against_float64():
    cl, R, nb, rgb, v, f, degenerate, T, f64, f32 = _scene()
    info = f64[2]
    c, n, b = texture_reference.layout(len(f), T)
    assert (c, n) == (7, 18) and not info["owned"][:, n * c:].any() and T - n * c == 2      # a 2-texel unowned strip remains
    assert info["face_distance"] > 1e-5                       # float32 and float64 agree about every member
    assert np.array_equal(info["keep"], f32[2]["keep"]) and np.array_equal(info["members"], f32[2]["members"])
    assert info["members"].max() > 2048                       # the member list is flushed in mid-walk
    counts = np.bincount(info["face_block"], minlength=nb ** 3)
    assert (counts == 0).any() and (counts == 1).any()
    # the crowded block: more than two workgroups' worth of one pass each, so slices = 3 splits it AND gives a slice a second pass
    assert counts.max() * texture_inputs.slots_per_face(c) > 2 * 3 * texture_inputs.ONE_PASS
    print("%d faces, %d owned texels, %d in the crowded block, up to %d members" %
          (len(f), info["owned"].sum(), np.bincount(info["face_block"][info["face"]]).max(), info["members"].max()))
    assert (np.abs(v) > 1).any()                              # vertices outside the grid
    gm = _model(cl, rgb)
    out = _bake(gm, v, f, T, colors=torch.from_numpy(rgb).cuda(), resolution=R, num_blocks=nb)
    assert out["cell"] == c and np.array_equal(out["uv"].cpu().numpy(), texture_reference.uv(len(f), T))
    _against_float64("parity", out, f64, f32)
    flat = torch.from_numpy(info["face"] == degenerate)       # the degenerate face: one point, so one value
    ys, xs = torch.from_numpy(info["y"])[flat].cuda(), torch.from_numpy(info["x"])[flat].cuda()
    d, cs = out["density"][ys, xs], out["color_sum"][ys, xs]
    assert len(d) in (c * (c + 1) // 2, c * (c - 1) // 2) and (d == d[0]).all() and (cs == cs[0]).all()
    # the public entry point: the blend of the same sums, 0 where nothing was summed
    baked = gm.bake_texture(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), T, colors=torch.from_numpy(rgb).cuda(), resolution=R,
                            num_blocks=nb, normalized=True)
    assert set(baked) == {"texture", "density", "uv", "cell"} and baked["texture"].shape == (T, T, 3)
    assert torch.equal(baked["density"], out["density"]) and torch.equal(baked["texture"], gm._blend(
        out["color_sum"].reshape(-1, 3), out["density"].reshape(-1)).reshape(T, T, 3))
    assert float(baked["texture"].min()) >= 0 and float(baked["texture"].max()) <= 1 + 1e-6
    assert not baked["texture"][out["density"] == 0].any()


# ---------------------------------------------------------------------------------------------------------------- 2. the sampler
def test_bitwise_equal_to_the_sampler():
    from gaussianip_amd.utils import texture as tex
    cl, R, nb, rgb, v, f, _, T, f64, _ = _scene()
    gm = _model(cl, rgb)
    colors = torch.from_numpy(rgb).cuda()
    out = _bake(gm, v, f, T, colors=colors, resolution=R, num_blocks=nb)
    pts, face, x, y = tex.texel_points(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), T)
    assert pts.is_cuda and len(pts) == int(f64[2]["owned"].sum())
    block = torch.from_numpy(f64[2]["face_block"]).cuda()[face]
    want = gm._sample("test", pts.contiguous(), block, colors, R, nb, 1.5)
    assert torch.equal(out["density"][y, x], want["density"])
    assert torch.equal(out["color_sum"][y, x], want["color_sum"])


# ---------------------------------------------------------------------------------------------------------------- 3. the split
def test_slices_do_not_change_the_result():
    cl, R, nb, rgb, v, f, _, T, _, _ = _scene()
    gm = _model(cl, rgb)
    kw = dict(colors=torch.from_numpy(rgb).cuda(), resolution=R, num_blocks=nb)
    auto = _bake(gm, v, f, T, **kw)
    for slices in (1, 3, None):
        other = _bake(gm, v, f, T, slices=slices, **kw)
        assert torch.equal(other["density"], auto["density"]) and torch.equal(other["color_sum"], auto["color_sum"]), slices
    assert float(auto["density"].max()) > 0
    with pytest.raises(ValueError):
        gm._bake_sums(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), T, slices=0, normalized=True, **kw)


# ---------------------------------------------------------------------------------------------------------------- 4. extremes
@pytest.mark.parametrize("F,T,c", [(1, 64, 64), (2, 64, 64), (7, 16, 8), (2 * (32 // 4) ** 2, 32, 4)])
def test_layout_extremes(F, T, c):
    cl, R, nb = field_inputs.case("b")
    rgb = sample_inputs.colors(cl["xyz"].shape[0], 5)
    v, f = texture_inputs.random_mesh(F, seed=100 + F)
    assert texture_reference.layout(F, T)[0] == c
    f64 = texture_reference.bake_sums(cl, rgb, R, nb, v, f, T, np.float64)
    f32 = texture_reference.bake_sums(cl, rgb, R, nb, v, f, T, np.float32)
    assert f64[2]["face_distance"] > 1e-5 and np.array_equal(f64[2]["members"], f32[2]["members"])
    if c == 4:
        assert f64[2]["owned"].all()                          # the atlas is full
    out = _bake(_model(cl, rgb), v, f, T, colors=torch.from_numpy(rgb).cuda(), resolution=R, num_blocks=nb)
    assert out["cell"] == c and float(out["density"].max()) > 0
    _against_float64("extreme_F%d_T%d" % (F, T), out, f64, f32)


def test_no_faces_and_nothing_passing_the_prefilter():
    cl, R, nb = field_inputs.case("b")
    gm = _model(cl)
    out = _bake(gm, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 64, launches=0, resolution=R, num_blocks=nb)
    assert not out["density"].any() and not out["color_sum"].any() and out["cell"] == 64
    baked = gm.bake_texture(torch.zeros((5, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int32, device="cuda"), resolution=R,
                            num_blocks=nb)
    assert baked["texture"].shape == (64, 64, 3) and not baked["texture"].any() and baked["uv"].shape == (0, 3, 2)
    cl, R, nb = field_inputs.edge_case("transparent")
    v, f = texture_inputs.random_mesh(20, seed=4)
    for normalized in (False, True):
        baked = _model(cl).bake_texture(torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda(), 32, resolution=R, num_blocks=nb,
                                        normalized=normalized)
        assert not baked["texture"].any() and not baked["density"].any()      # colour 0, not NaN


def test_argument_errors():
    cl, R, nb = field_inputs.edge_case("single")
    gm = _model(cl)
    v, f = (torch.from_numpy(t).cuda() for t in texture_inputs.random_mesh(20, seed=4))
    kw = dict(resolution=R, num_blocks=nb)
    with pytest.raises(ValueError):
        gm.bake_texture(v.cpu(), f, 32, **kw)                 # not on the GPU
    with pytest.raises(ValueError):
        gm.bake_texture(v, f.long(), 32, **kw)                # not int32
    with pytest.raises(ValueError):
        gm.bake_texture(v[:, :2], f, 32, **kw)
    with pytest.raises(ValueError, match="divide"):
        gm.bake_texture(v, f, 32, resolution=30, num_blocks=16)
    with pytest.raises(ValueError):
        gm.bake_texture(v, f, 32, colors=torch.zeros((5, 3), device="cuda"), **kw)
    with pytest.raises(ValueError, match="16"):               # 20 faces need 4 cells per row: 16 texels
        gm.bake_texture(v, f, 12, **kw)
    bad = f.clone()
    bad[7, 1] = v.shape[0]
    with pytest.raises(ValueError, match="indices"):
        gm.bake_texture(v, bad, 32, **kw)
    bad[7, 1] = -1
    with pytest.raises(ValueError, match="indices"):
        gm.bake_texture(v, bad, 32, **kw)


# ---------------------------------------------------------------------------------------------------------------- 5. one Gaussian
def test_one_isotropic_gaussian():
    cl, rgb = sample_inputs.sphere_cloud()
    gm = _model(cl, rgb)
    kw = dict(density_thresh=sample_inputs.SPHERE_THRESHOLD, resolution=32, num_blocks=4)
    v, f, n, uv, texture = gm.extract_textured_mesh(**kw)
    v0, f0, n0, _ = _model(cl, rgb).extract_mesh_with_attributes(**kw)
    assert torch.equal(v, v0) and torch.equal(f, f0) and torch.equal(n, n0) and f.shape[0] > 100
    T = texture.shape[0]
    assert texture.shape == (T, T, 3) and T >= 64 and T & (T - 1) == 0 and uv.shape == (f.shape[0], 3, 2)
    assert texture_reference.layout(f.shape[0], T)[0] >= 8 and (T == 64 or texture_reference.layout(f.shape[0], T // 2)[0] < 8)
    assert np.array_equal(uv.cpu().numpy(), texture_reference.uv(f.shape[0], T))
    # corners, edge midpoints and barycentre of every face: a single unfilled or foreign texel in any footprint breaks this
    got = texture_reference.bilinear(texture.cpu().numpy(), texture_inputs.face_samples(uv.cpu().numpy()))
    cerr = np.abs(got - np.array(sample_inputs.SPHERE_COLOR, np.float32).astype(np.float64)).max()
    print("%d faces, texture %d, colour error %.3e" % (f.shape[0], T, cerr))
    _figures["sphere_colour_err"] = float(cerr)
    assert cerr <= 1e-5


# ---------------------------------------------------------------------------------------------------------------- 6. end to end
def test_textured_mesh_end_to_end(tmp_path):
    from gaussianip_amd.utils.mesh import read_obj_textured
    cl = sample_inputs.blob_cloud()
    rgb = sample_inputs.colors(cl["xyz"].shape[0], 9)
    R, nb, thr = 64, 8, 1.0
    gm = _model(cl, rgb)
    obj = tmp_path / "out" / "avatar.obj"
    v, f, n, uv, texture = gm.extract_textured_mesh(path=str(obj), density_thresh=thr, resolution=R, num_blocks=nb)
    v0, f0 = gm.extract_mesh(density_thresh=thr, resolution=R, num_blocks=nb)
    assert torch.equal(v, v0) and torch.equal(f, f0) and f.shape[0] > 1000
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["avatar.mtl", "avatar.obj", "avatar_kd.png"]
    rv, rf, rn, ruv, rtex = read_obj_textured(str(obj))
    assert np.array_equal(rv, v.cpu().numpy()) and np.array_equal(rf, f.cpu().numpy()) and np.array_equal(rn, n.cpu().numpy())
    assert np.array_equal(ruv, uv.cpu().numpy())
    assert rtex.shape == tuple(texture.shape) and np.abs(rtex - texture.cpu().numpy()).max() <= 0.5 / 255 + 1e-7
    assert float(texture.min()) >= 0 and float(texture.max()) <= 1 + 1e-6
    # The bilinear lookup at a face's barycentre against the field sampled there.  The lookup is a convex combination of the four
    # texels around the barycentre, each the blend at its own point of the face's plane in the face's block; so it differs from the
    # blend at the barycentre by no more than the farthest of those four does (plus rounding: 1e-5, the colour bar of the sphere test).
    T, F = texture.shape[0], f.shape[0]
    c, _, b = texture_reference.layout(F, T)
    u = (v - gm.center) * gm.scale
    tri = u[f.long()]
    bary = (tri[:, 0] + tri[:, 1] + tri[:, 2]) / 3
    grid = torch.linspace(-1, 1, R, dtype=torch.float32).cuda()
    cell = (torch.bucketize(bary.contiguous(), grid, right=True) - 1).clamp(0, R - 1) // (R // nb)
    block = (cell[:, 0] * nb + cell[:, 1]) * nb + cell[:, 2]
    pts = [bary]
    for li in (b // 3, b // 3 + 1):
        for lj in (b // 3, b // 3 + 1):
            pts.append(tri[:, 0] + (li / b) * (tri[:, 1] - tri[:, 0]) + (lj / b) * (tri[:, 2] - tri[:, 0]))
    out = gm._sample("test", torch.cat(pts).contiguous(), block.repeat(5), None, R, nb, 1.5)
    col = gm._blend(out["color_sum"], out["density"]).reshape(5, F, 3).cpu().numpy().astype(np.float64)
    assert float(out["density"].min()) > 0
    spread = np.abs(col[1:] - col[0]).max(0)                                   # [F, 3]
    look = texture_reference.bilinear(texture.cpu().numpy(), texture_inputs.face_samples(uv.cpu().numpy())[:, 6])
    diff = np.abs(look - col[0])
    print("%d faces, texture %d (cell %d): lookup - sample at the barycentre at most %.3e, the four texels' spread at most %.3e (median "
          "%.3e)" % (F, T, c, diff.max(), spread.max(), np.median(spread)))
    assert (diff <= spread + 1e-5).all()
