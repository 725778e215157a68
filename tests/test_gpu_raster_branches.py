"""Branches of preprocess.hip / gather_backward.hip / render_backward.hip that the other rasterizer tests do not reach, against the
CPU oracle, which tests/test_oracle_vs_dense.py pins to the float64 autograd model on the very same scenes:

  1. Gaussians on the clamped side of the Jacobian's 1.3 x tanfov clamp (the backward's xmul / ymul) and behind the near plane;
  2. the same, differing from view to view inside one launch set (both SH paths);
  3. scale_modifier != 1, whose scale gradient is taken with respect to modifier * scale (the fork's quirk);
  4. every non-empty subset of (colour, depth, alpha) as the upstream gradients: the absent ones reach the kernels as NULL;
  5. sizes on the edges of the launch geometry: P around the 256-Gaussian scan block and the 1024-lane preprocess workgroup,
     images smaller than one 8 x 8 quadrant of a tile, markVisible past a block;
  6. every call twice in a row with one shape: the first in the dense key layout, the second in buckets (rasterizer.py, "Key
     layout"), outputs and gradients bit for bit the same.

Bars: those of test_gpu_raster_parity.py (`_check_forward_scene`, `_check_backward`: 2e-3 of the largest gradient per tensor with
the backward isolated through the implementation's own alpha image, 5e-3 end to end); 1e-5 between two paths that differ by
rounding only, as in test_multiview_equals_single_views."""
import numpy as np
import pytest
import torch

import scenes
from antialias_reference import composite_grads, effective_opacities, scene_compensation
from dense_reference import _quat_to_rot, clamp_cull_masks, random_scene
from test_gpu_raster_parity import _assert_images, _check_backward, _check_forward_scene, _dev, _oracle_forward, _settings
from test_oracle_vs_dense import FLOORS, SCENE_A, SCENE_B, SCENE_MOD, SCENE_SUBSETS, SUBSETS

pytestmark = pytest.mark.gpu

BG = (0.3, 0.1, 0.2)
DEFAULT_CAM = (10.0, 40.0, 1.6, 60.0)           # test_oracle_vs_dense._run's
GRADS = ("means3D", "opacities", "shs", "scales", "rotations")
ISO_TOL = 2e-3                                  # _check_backward's bar with the backward isolated
ROUNDING_TOL = 1e-5


@pytest.fixture
def plans(monkeypatch):
    """Every plan that goes through the forward launcher, in order (plan.bucket_stride says which layout it used)."""
    from gaussianip_amd import rasterizer as R
    seen = []
    orig = R._run_forward

    def spy(plan, *a, **k):
        seen.append(plan)
        return orig(plan, *a, **k)
    monkeypatch.setattr(R, "_run_forward", spy)
    monkeypatch.delenv("GIP_RASTER_BUCKET_BYTES", raising=False)
    return seen


def _scene(spec):
    """(float64 scene, the same rounded to float32 numpy, numpy camera) of a scene description of test_oracle_vs_dense.py."""
    sc64 = random_scene(spec["P"], spec["seed"], sh_M=(spec["sh_degree"] + 1) ** 2, **spec.get("scene_kw", {}))
    sc = {k: v.numpy().astype(np.float32) for k, v in sc64.items()}
    return sc64, sc, scenes.camera(*spec.get("cam", DEFAULT_CAM), spec["H"], spec["W"])


def _both_layouts(monkeypatch, plans, call):
    """call() twice in a row.  The first call of a shape is dense; it is forced dense here, because an earlier test may have
    left the shape its hint.  The second finds the hint the first one left and must run in buckets.  Returns both results."""
    res = []
    for buckets in ("0", "1"):
        monkeypatch.setenv("GIP_RASTER_BUCKETS", buckets)
        n = len(plans)
        res.append(call())
        strides = [p.bucket_stride for p in plans[n:]]
        assert strides and all((s != 0) == (buckets == "1") for s in strides), (buckets, strides)
    return res


def _same(a, b, what):
    assert (a is None and b is None) or torch.equal(a, b), "%s differs between the dense and the bucket layout" % what


def _backward_both_layouts(oracle, monkeypatch, plans, sc, cam, H, W, deg, **kw):
    """_check_backward in both key layouts; gradients, images and radii of the two are bit-identical.
    Returns ({input: gradient tensor}, the `outputs` of the first call)."""
    P = sc["means3D"].shape[0]
    outs = []

    def call():
        outs.append({})
        return _check_backward(oracle, None, P, H, W, 0, deg, scene=sc, cam=cam, outputs=outs[-1], **kw)
    (t0, m0), (t1, m1) = _both_layouts(monkeypatch, plans, call)
    g0, g1 = ({**{k: v.grad for k, v in t.items()}, "means2D": m.grad} for t, m in ((t0, m0), (t1, m1)))
    for k in g0:
        _same(g0[k], g1[k], k)
    for k in ("color", "radii", "depth", "alpha", "colors_precomp", "cov3D_precomp"):
        _same(outs[0][k], outs[1][k], k)
        if k.endswith("precomp") and outs[0][k] is not None:
            g0[k] = outs[0][k]
    return {k: v for k, v in g0.items() if v is not None}, outs[0]


def _forward_both_layouts(oracle, monkeypatch, plans, sc, cam, H, W, deg, **kw):
    outs = []

    def call():
        outs.append({})
        return _check_forward_scene(oracle, sc, cam, H, W, deg, BG, outputs=outs[-1], **kw)
    _both_layouts(monkeypatch, plans, call)
    for k in ("color", "radii", "depth", "alpha"):
        _same(outs[0][k], outs[1][k], k)
    assert outs[0]["plan"].bucket_stride == 0 and outs[1]["plan"].bucket_stride != 0      # through forward_with_state
    return outs[0]


def _cov_of(sc64, modifier=1.0):
    """[P,6] float32 covariances of the float64 scene, of modifier * scales."""
    L = _quat_to_rot(sc64["rotations"]) * (modifier * sc64["scales"])[:, None, :]
    S = L @ L.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], dim=1).numpy().astype(np.float32)


def _rel(ours, ref, floor=0.0):
    ours = ours.detach().cpu().numpy().reshape(np.shape(ref)).astype(np.float64)
    return float(np.abs(ours - ref).max() / (max(float(np.abs(ref).max()), floor) + 1e-20))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. clamp and cull, single view
# ---------------------------------------------------------------------------------------------------------------------------
def _assert_populations(name, clamped, behind, radii, ref_means3D):
    vis = clamped & (radii > 0)
    pops = (int(vis.sum()), int((vis & (np.abs(ref_means3D).max(1) > 0)).sum()), int(behind.sum()))
    print("scene %s: clamped and visible %d, with a gradient %d, behind the near plane %d" % ((name,) + pops))
    assert all(p >= f for p, f in zip(pops, FLOORS[name])), (pops, FLOORS[name])


def _assert_zero_rows(grads, rows):
    assert rows.any()
    for k, g in grads.items():
        assert float(g[torch.from_numpy(rows).to(g.device)].abs().max()) == 0.0, "%s: a culled Gaussian's row is not exactly zero" % k


@pytest.mark.parametrize("precomp", [False, True], ids=["scale-rotation-sh", "precomputed"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_clamped_and_culled_gaussians(oracle, monkeypatch, plans, name, precomp):
    """Scenes A and B (B at scale_modifier 1.5) of test_oracle_vs_dense.py: radii and records bit-exact, images and every gradient
    at the parity bars, exact zeros for the Gaussians behind the near plane; with scales / rotations / SH and with precomputed
    colours and covariances (the covariance gradient's write-out)."""
    spec = SCENE_A if name == "A" else SCENE_B
    sc64, sc, cam = _scene(spec)
    H, W, deg, mod = spec["H"], spec["W"], spec["sh_degree"], spec.get("scale_modifier", 1.0)
    clamped, behind = clamp_cull_masks(sc["means3D"], cam["viewmatrix"], cam["tanfovx"], cam["tanfovy"])
    if not precomp:
        # min_keep: the plausibility floor of the instance culling does not hold for large translucent splats (opacity 0.02:
        # the alpha >= 1/255 region ends at 1.8 sigma, the rectangle at 3); every dropped entry is still proven dead
        fwd = _forward_both_layouts(oracle, monkeypatch, plans, sc, cam, H, W, deg, scale_modifier=mod, min_keep=0.0)
        assert not fwd["radii"][0].cpu().numpy()[behind].any()
    grads, out = _backward_both_layouts(oracle, monkeypatch, plans, sc, cam, H, W, deg, scale_modifier=mod, use_precomp=precomp,
                                        cov=_cov_of(sc64, mod) if precomp else None)
    radii = out["radii"].cpu().numpy()
    assert np.array_equal(radii, out["oracle_radii"]), "radii"
    _assert_populations(name, clamped, behind, radii, out["oracle_grads"]["means3D"])
    assert set(grads) == ({"means3D", "means2D", "opacities", "colors_precomp", "cov3D_precomp"} if precomp else
                          {"means3D", "means2D", "opacities", "shs", "scales", "rotations"})
    _assert_zero_rows(grads, behind)


def test_clamped_and_culled_gaussians_antialiased(oracle, monkeypatch, plans):
    """Scene A with the opacity compensation: its derivative sits in the same block of gather_backward.hip as the clamp's.
    Reference: the composite oracle (tests/antialias_reference.py, pinned to the dense model on this scene by
    test_antialias_cpu.py), as in test_gpu_antialias.py: rows of proven knife-edge Gaussians are left out, because the kernels
    compute the compensation in float32 and the reference in float64."""
    from gaussianip_amd import GaussianRasterizer
    spec = SCENE_A
    _, sc, cam = _scene(spec)
    P, H, W, deg = spec["P"], spec["H"], spec["W"], spec["sh_degree"]
    clamped, behind = clamp_cull_masks(sc["means3D"], cam["viewmatrix"], cam["tanfovx"], cam["tanfovy"])
    rng = np.random.default_rng(5)
    ups = [rng.normal(size=(c, H, W)).astype(np.float32) for c in (3, 1, 1)]
    st = _settings(cam, H, W, BG, deg)._replace(antialiasing=True)

    def call():
        t = {k: _dev(v).requires_grad_(True) for k, v in sc.items()}
        t["means2D"] = torch.zeros(P, 3, device="cuda", requires_grad=True)
        outs = GaussianRasterizer(st)(**t)
        sum((o * _dev(g)).sum() for o, g in zip((outs[0], outs[2], outs[3]), ups)).backward()
        torch.cuda.synchronize()
        return [o.detach() for o in outs], {k: v.grad for k, v in t.items()}
    (outs, g), (outs1, g1) = _both_layouts(monkeypatch, plans, call)
    for k in g:
        _same(g[k], g1[k], k)
    for a, b in zip(outs, outs1):
        _same(a, b, "an output")
    color, radii, depth, alpha = outs
    comp, _ = scene_compensation(sc, cam, H, W)
    assert int((clamped & (comp.numpy() < 0.999)).sum()) >= FLOORS["A"][0]
    ro, (o_color, o_radii, o_depth, o_alpha) = _oracle_forward(oracle, dict(sc, opacities=effective_opacities(sc, comp)), cam, H, W, BG, deg)
    assert np.array_equal(radii.cpu().numpy(), o_radii)
    _assert_images(ro, color, depth, alpha, o_color, o_depth, o_alpha)
    go = ro.backward(*ups, alpha_out=alpha.cpu().numpy())
    ref = composite_grads(go, sc, cam, H, W, fork_clamp=True)
    knife = ro.knife_edge_gaussians()[0]
    _assert_populations("A", clamped & ~knife, behind, radii.cpu().numpy(), ref["means3D"])
    floor = float(np.abs(ref["scales"] * sc["scales"]).max())
    for k in ("means2D",) + GRADS:
        ours = g[k].cpu().numpy().reshape(ref[k].shape).astype(np.float64)
        ours[knife] = ref[k][knife]
        err = _rel(torch.from_numpy(ours), ref[k], floor if k == "rotations" else 0.0)
        print("antialiased %s: %.2e" % (k, err))
        assert err < ISO_TOL, "%s: max error / max |grad| = %.3e" % (k, err)
    _assert_zero_rows(g, behind)


# ---------------------------------------------------------------------------------------------------------------------------
# 2. clamped / culled in some views of a launch set only
# ---------------------------------------------------------------------------------------------------------------------------
VIEW_CAMS = [(10.0, 40.0, 0.9, 50.0), (-20.0, 160.0, 1.0, 50.0), (35.0, -80.0, 0.8, 50.0)]


@pytest.mark.parametrize("sh_path", ["scalar", "matrix cores"])
def test_per_view_clamp_and_cull_in_one_launch_set(oracle, monkeypatch, plans, sh_path):
    from gaussianip_amd import rasterize_views
    monkeypatch.setenv("GIP_RASTER_SH_SCALAR", "1" if sh_path == "scalar" else "0")
    spec = SCENE_A
    _, sc, _ = _scene(spec)
    P, H, W, deg, V = spec["P"], spec["H"], spec["W"], spec["sh_degree"], len(VIEW_CAMS)
    cams = [scenes.camera(*c, H, W) for c in VIEW_CAMS]
    masks = [clamp_cull_masks(sc["means3D"], c["viewmatrix"], c["tanfovx"], c["tanfovy"]) for c in cams]
    clamped, behind = np.stack([m[0] for m in masks]), np.stack([m[1] for m in masks])
    n_clamp, n_cull = int((clamped.any(0) & ~clamped.all(0)).sum()), int((behind.any(0) & ~behind.all(0)).sum())
    print("clamped in some views only: %d, culled in some views only: %d" % (n_clamp, n_cull))
    assert n_clamp >= 60 and n_cull >= 25
    rng = np.random.default_rng(17)
    ups = [rng.normal(size=(V, c, H, W)).astype(np.float32) for c in (3, 1, 1)]
    sts = [_settings(c, H, W, BG, deg) for c in cams]

    def call():
        t = {k: _dev(v).requires_grad_(True) for k, v in sc.items()}
        m2 = torch.zeros(V, P, 3, device="cuda", requires_grad=True)
        outs = rasterize_views(t["means3D"], m2, t["opacities"], sts, shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
        sum((o * _dev(g)).sum() for o, g in zip((outs[0], outs[2], outs[3]), ups)).backward()
        torch.cuda.synchronize()
        return [o.detach() for o in outs], {**{k: v.grad for k, v in t.items()}, "means2D": m2.grad}
    (outs, g), (outs1, g1) = _both_layouts(monkeypatch, plans, call)
    assert plans[-1].cfg.sh_scalar == (1 if sh_path == "scalar" else 0)
    for k in g:
        _same(g[k], g1[k], k)
    for a, b in zip(outs, outs1):
        _same(a, b, "an output")
    color, radii, depth, alpha = outs
    refs = []
    for v, cam in enumerate(cams):
        ro, (o_color, o_radii, o_depth, o_alpha) = _oracle_forward(oracle, sc, cam, H, W, BG, deg)
        assert np.array_equal(radii[v].cpu().numpy(), o_radii), "radii of view %d" % v
        assert not o_radii[behind[v]].any() and (o_radii[clamped[v]] > 0).any()
        _assert_images(ro, color[v], depth[v], alpha[v], o_color, o_depth, o_alpha)
        go = ro.backward(ups[0][v], ups[1][v], ups[2][v], alpha_out=alpha[v].cpu().numpy())
        err = _rel(g["means2D"][v], go["means2D"])
        assert err < ISO_TOL, "means2D of view %d: %.3e" % (v, err)
        assert float(g["means2D"][v][torch.from_numpy(behind[v]).cuda()].abs().max()) == 0.0
        refs.append(go)
    tot = {k: sum(go[k].astype(np.float64) for go in refs) for k in GRADS}
    floor = float(np.abs(tot["scales"] * sc["scales"]).max())
    for k in GRADS:
        err = _rel(g[k], tot[k], floor if k == "rotations" else 0.0)
        print("%s SH, %s: %.2e" % (sh_path, k, err))
        assert err < ISO_TOL, "%s: max error / max |summed grad| = %.3e" % (k, err)
    if behind.all(0).any():
        _assert_zero_rows({k: g[k] for k in GRADS}, behind.all(0))


# ---------------------------------------------------------------------------------------------------------------------------
# 3. scale_modifier != 1
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("modifier", [0.5, 2.5])
def test_scale_modifier(oracle, monkeypatch, plans, modifier):
    spec = SCENE_MOD
    _, sc, cam = _scene(spec)
    H, W, deg = spec["H"], spec["W"], spec["sh_degree"]
    fwd = _forward_both_layouts(oracle, monkeypatch, plans, sc, cam, H, W, deg, scale_modifier=modifier, min_keep=0.0)
    assert int((fwd["radii"] > 0).sum()) >= spec["P"] // 2 and float(fwd["alpha"].max()) < 0.999
    grads, _ = _backward_both_layouts(oracle, monkeypatch, plans, sc, cam, H, W, deg, scale_modifier=modifier)
    # the quirk, stated directly: the scale gradient is the one with respect to modifier * scale, i.e. what a call with the
    # scales premultiplied and modifier 1 returns (0.5 and 2.5 are exact in float32: the kernels see the same products)
    pre = dict(sc, scales=(np.float32(modifier) * sc["scales"]).astype(np.float32))
    t, m2 = _check_backward(oracle, None, spec["P"], H, W, 0, deg, scene=pre, cam=cam)
    assert float(grads["scales"].abs().max()) > 0
    for k in GRADS:
        ref = t[k].grad
        err = float((grads[k] - ref).abs().max() / ref.abs().max())
        assert err < ROUNDING_TOL, "%s at modifier %g against premultiplied scales: %.3e" % (k, modifier, err)


# ---------------------------------------------------------------------------------------------------------------------------
# 4. subsets of the upstream gradients
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("upstream", SUBSETS, ids=["+".join(s) for s in SUBSETS])
def test_upstream_gradient_subsets(oracle, monkeypatch, plans, upstream):
    spec = SCENE_SUBSETS
    _, sc, cam = _scene(spec)
    grads, _ = _backward_both_layouts(oracle, monkeypatch, plans, sc, cam, spec["H"], spec["W"], spec["sh_degree"], upstream=upstream)
    assert float(grads["means3D"].abs().max()) > 0
    assert (float(grads["shs"].abs().max()) > 0) == ("color" in upstream)


def test_upstream_gradients_are_linear():
    """The gradients under colour, depth and alpha alone add up to the gradient under all three."""
    from gaussianip_amd import GaussianRasterizer
    spec = SCENE_SUBSETS
    _, sc, cam = _scene(spec)
    P, H, W = spec["P"], spec["H"], spec["W"]
    st = _settings(cam, H, W, BG, spec["sh_degree"])
    gen = torch.Generator(device="cuda").manual_seed(4)
    ups = [torch.randn(c, H, W, device="cuda", generator=gen) for c in (3, 1, 1)]

    def grads(which):
        t = {k: _dev(v).requires_grad_(True) for k, v in sc.items()}
        t["means2D"] = torch.zeros(P, 3, device="cuda", requires_grad=True)
        outs = GaussianRasterizer(st)(**t)
        outs = (outs[0], outs[2], outs[3])
        return dict(zip(t, torch.autograd.grad([outs[i] for i in which], list(t.values()), [ups[i] for i in which])))
    whole = grads((0, 1, 2))
    parts = [grads((i,)) for i in range(3)]
    for k, ref in whole.items():
        err = float((sum(p[k] for p in parts) - ref).abs().max() / ref.abs().max())
        assert err < ROUNDING_TOL, "%s: %.3e" % (k, err)


# ---------------------------------------------------------------------------------------------------------------------------
# 5. size edges of the launch geometry
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 255, 257, 1023, 1025])
def test_gaussian_counts_around_the_block_sizes(oracle, monkeypatch, plans, P):
    spec = dict(P=P, seed=20 + P % 7, sh_degree=0, H=32, W=32)
    _, sc, cam = _scene(spec)
    fwd = _forward_both_layouts(oracle, monkeypatch, plans, sc, cam, 32, 32, 0)
    assert int((fwd["radii"] > 0).sum()) >= max(1, P // 2)
    grads, _ = _backward_both_layouts(oracle, monkeypatch, plans, sc, cam, 32, 32, 0)
    assert float(grads["means3D"].abs().max()) > 0


@pytest.mark.parametrize("H,W", [(3, 5), (8, 9), (17, 33)])
def test_images_smaller_than_a_tile_quadrant(oracle, monkeypatch, plans, H, W):
    """3 x 5: inside one 8 x 8 quadrant; 8 x 9: one column into the next quadrant; 17 x 33: a second tile row of one pixel row and
    a third tile column of one pixel column."""
    spec = dict(P=40, seed=9, sh_degree=1, H=H, W=W)
    _, sc, cam = _scene(spec)
    fwd = _forward_both_layouts(oracle, monkeypatch, plans, sc, cam, H, W, 1)
    assert int((fwd["radii"] > 0).sum()) >= 20
    grads, _ = _backward_both_layouts(oracle, monkeypatch, plans, sc, cam, H, W, 1)
    assert float(grads["means3D"].abs().max()) > 0


def test_mark_visible_past_a_block():
    """markVisible on 1025 points (four full 256-lane blocks and one lane): the fork's view-space z > 0.2, in float32 and in the
    kernel's order of operations (preprocess.hip is compiled without contraction)."""
    from gaussianip_amd import GaussianRasterizer
    spec = SCENE_A
    _, sc, cam = _scene(spec)
    pts = np.resize(sc["means3D"], (1025, 3)).astype(np.float32)
    v = cam["viewmatrix"].reshape(-1)
    z = ((v[2] * pts[:, 0] + v[6] * pts[:, 1]) + v[10] * pts[:, 2]) + v[14]
    assert z.dtype == np.float32
    expect = z > np.float32(0.2)
    assert int(expect.sum()) >= 10 and int((~expect).sum()) >= 10
    vis = GaussianRasterizer(_settings(cam, spec["H"], spec["W"], BG, 0)).markVisible(_dev(pts))
    assert vis.dtype == torch.bool and vis.shape == (1025,)
    assert np.array_equal(vis.cpu().numpy(), expect)
