"""The CPU oracle (oracle/raster_oracle.c) against an independent dense float64 autograd model
(tests/dense_reference.py): forward images, integer buffers, and every gradient."""
import numpy as np
import pytest
import torch

from dense_reference import clamp_cull_masks, dense_render, look_at_camera, random_scene


def _run(oracle, P, H, W, seed, sh_degree=0, use_cov=False, use_colors=False, bgval=(0.2, 0.5, 0.9), cam=(10.0, 40.0, 1.6, 60.0),
         scene_kw=None, scale_modifier=1.0, fork_clamp=False):
    """`scale_modifier` goes to both models; `fork_clamp` to the dense one (dense_render: the fork's derivative of the clamp)."""
    M = (sh_degree + 1) ** 2
    sc = random_scene(P, seed, sh_M=M, **(scene_kw or {}))
    view, proj, campos, tanx, tany = look_at_camera(cam[0], cam[1], cam[2], cam[3], H, W)
    bg = torch.tensor(bgval, dtype=torch.float64)
    leaves = {k: v.clone().requires_grad_(True) for k, v in sc.items()}
    means2D = torch.zeros(P, 3, dtype=torch.float64, requires_grad=True)
    kw = dict(means3D=leaves["means3D"], opacities=leaves["opacities"], viewmatrix=view, projmatrix=proj, campos=campos,
              bg=bg, H=H, W=W, tanfovx=tanx, tanfovy=tany, sh_degree=sh_degree, means2D=means2D,
              scale_modifier=scale_modifier, fork_clamp=fork_clamp)
    okw = dict(image_height=H, image_width=W, tanfovx=tanx, tanfovy=tany, bg=bg.numpy(), scale_modifier=scale_modifier,
               viewmatrix=view.numpy(), projmatrix=proj.numpy(), sh_degree=sh_degree, campos=campos.numpy(),
               means3D=sc["means3D"].numpy(), opacities=sc["opacities"].numpy())
    cov_leaf = col_leaf = None
    if use_cov:
        from dense_reference import _quat_to_rot
        R = _quat_to_rot(sc["rotations"])
        L = R * sc["scales"][:, None, :]
        S = L @ L.transpose(1, 2)
        cov = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], dim=1)
        cov_leaf = cov.clone().requires_grad_(True)
        kw["cov3D_precomp"] = cov_leaf
        okw["cov3D_precomp"] = cov.numpy()
    else:
        kw.update(scales=leaves["scales"], rotations=leaves["rotations"])
        okw.update(scales=sc["scales"].numpy(), rotations=sc["rotations"].numpy())
    if use_colors:
        g = torch.Generator().manual_seed(seed + 1)
        col = torch.rand(P, 3, generator=g, dtype=torch.float64)
        col_leaf = col.clone().requires_grad_(True)
        kw["colors_precomp"] = col_leaf
        okw["colors_precomp"] = col.numpy()
    else:
        kw["shs"] = leaves["shs"]
        okw["shs"] = sc["shs"].numpy()
    out = dense_render(**kw)
    ro = oracle.RasterOracle()
    color, radii, depth, alpha = ro.forward(**okw)
    return sc, leaves, means2D, cov_leaf, col_leaf, out, ro, (color, radii, depth, alpha)


@pytest.mark.parametrize("P,H,W,seed,deg", [(64, 32, 48, 1, 0), (150, 64, 64, 2, 1), (100, 40, 56, 3, 3), (200, 64, 80, 4, 2)])
def test_forward_matches_dense(oracle, P, H, W, seed, deg):
    sc, leaves, m2d, _, _, out, ro, (color, radii, depth, alpha) = _run(oracle, P, H, W, seed, sh_degree=deg)
    assert np.array_equal(radii, out["radii"].numpy())
    keys, vals, ranges, tt, nc = ro.binning()
    assert np.array_equal(tt.astype(np.int64), out["tiles_touched"].numpy())
    assert ro.num_rendered == int(out["tiles_touched"].sum())
    np.testing.assert_allclose(color, out["color"].detach().numpy(), atol=2e-5)
    np.testing.assert_allclose(depth, out["depth"].detach().numpy(), atol=2e-5)
    np.testing.assert_allclose(alpha, out["alpha"].detach().numpy(), atol=2e-5)
    assert np.array_equal(nc.astype(np.int64), out["n_contrib"].numpy())
    # per-tile lists: sorted by depth then index; ranges tile the key array
    tiles_x = (W + 15) // 16
    depths = ro.geom()["depths"]
    for t in range(ranges.shape[0]):
        a, b = ranges[t]
        if b > a:
            assert np.all((keys[a:b] >> np.uint64(32)) == t)
            d = depths[vals[a:b]]
            assert np.all(np.diff(d) >= 0)
            same = np.diff(d) == 0
            assert np.all(np.diff(vals[a:b].astype(np.int64))[same] > 0)
    assert int((ranges[:, 1] - ranges[:, 0]).sum()) == ro.num_rendered


def _grad_check(oracle, **kwargs):
    _grad_compare(_run(oracle, **kwargs))


GRAD_RTOL = 2e-3
UPSTREAM = ("color", "depth", "alpha")


def _grad_errors(run, upstream=UPSTREAM, scale_modifier=1.0):
    """Backward of both models under random upstream gradients of the outputs named in `upstream`; an absent one reaches the
    oracle as None and is left out of the dense model's loss.  Returns ({tensor: max error / max |reference gradient|},
    {tensor: reference gradient}).  The oracle returns the scale gradient with respect to scale_modifier * scale (the fork's
    quirk, raster_oracle.c: cov3D_backward), the dense model differentiates the raw scales: oracle * modifier == dense."""
    sc, leaves, m2d, cov_leaf, col_leaf, out, ro, (color, radii, depth, alpha) = run
    H, W = color.shape[1:]
    g = torch.Generator().manual_seed(99)
    ups = {k: torch.randn(c, H, W, generator=g, dtype=torch.float64) for k, c in zip(UPSTREAM, (3, 1, 1))}
    names = {"means3D": leaves["means3D"], "means2D": m2d, "opacities": leaves["opacities"]}
    if cov_leaf is not None:
        names["cov3D_precomp"] = cov_leaf
    else:
        names.update(scales=leaves["scales"], rotations=leaves["rotations"])
    if col_leaf is not None:
        names["colors_precomp"] = col_leaf
    else:
        names["shs"] = leaves["shs"]
    loss = sum((out[k] * ups[k]).sum() for k in upstream)
    grads = torch.autograd.grad(loss, list(names.values()), retain_graph=True, allow_unused=True)
    ref = {k: (torch.zeros_like(t) if gr is None else gr).numpy() for (k, t), gr in zip(names.items(), grads)}
    go = ro.backward(*(ups[k].numpy() if k in upstream else None for k in UPSTREAM))
    errs = {}
    for k, r in ref.items():
        ours = go[k]
        if k == "means2D":
            ours, r = ours[:, :2], r[:, :2]
        elif k == "scales":
            ours = ours * scale_modifier
        errs[k] = float(np.abs(ours - r).max() / (np.abs(r).max() + 1e-12))
    return errs, ref


def _grad_compare(run, upstream=UPSTREAM, scale_modifier=1.0):
    errs, ref = _grad_errors(run, upstream, scale_modifier)
    print("worst rel-to-max error %.2e (%s)" % (max(errs.values()), " ".join("%s %.1e" % kv for kv in errs.items())))
    for name, err in errs.items():
        assert err < GRAD_RTOL, "%s: rel-to-max error %.3e" % (name, err)
    return errs, ref


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_backward_matches_autograd_sh(oracle, deg):
    _grad_check(oracle, P=80, H=48, W=48, seed=10 + deg, sh_degree=deg)


def test_backward_matches_autograd_precomp(oracle):
    _grad_check(oracle, P=90, H=48, W=64, seed=21, use_cov=True, use_colors=True)


def test_backward_black_bg_dense_scene(oracle):
    _grad_check(oracle, P=300, H=64, W=64, seed=33, sh_degree=0, bgval=(0.0, 0.0, 0.0), cam=(5.0, 90.0, 1.8, 70.0))


def test_deep_one_tile_list_matches_dense(oracle):
    """One 16 x 16 tile under 2400 large, nearly transparent Gaussians: a list of 2400 entries that the pixels walk to its
    end (median n_contrib above 2300) with the image still translucent.  The oracle is the reference of the GPU tests on
    long and deep tile lists (test_gpu_deep_lists.py); here its own images and every gradient are pinned to the dense
    float64 autograd model at this file's tolerances, thousands of blended entries per pixel included."""
    run = _run(oracle, P=2400, H=16, W=16, seed=7, sh_degree=1, cam=(10.0, 40.0, 1.6, 40.0),
               scene_kw=dict(scale_lo=0.2, scale_hi=0.6, opa_lo=0.0045, opa_hi=0.0075))
    sc, leaves, m2d, _, _, out, ro, (color, radii, depth, alpha) = run
    keys, vals, ranges, tt, nc = ro.binning()
    assert ranges.shape[0] == 1 and int(ranges[0, 1]) - int(ranges[0, 0]) >= 2048, ranges
    assert float(np.median(nc)) > 1024, float(np.median(nc))
    assert np.array_equal(radii, out["radii"].numpy())
    assert np.array_equal(tt.astype(np.int64), out["tiles_touched"].numpy())
    assert np.array_equal(nc.astype(np.int64), out["n_contrib"].numpy())
    np.testing.assert_allclose(color, out["color"].detach().numpy(), atol=2e-5)
    np.testing.assert_allclose(depth, out["depth"].detach().numpy(), atol=2e-5)
    np.testing.assert_allclose(alpha, out["alpha"].detach().numpy(), atol=2e-5)
    _grad_compare(run)


# ---------------------------------------------------------------------------------------------------------------------------
# The off-screen clamp of the Jacobian, the near cull, scale_modifier != 1 and partial upstream gradients.  The scenes are
# shared with tests/test_gpu_raster_branches.py, which holds the HIP kernels to the oracle on the same branches.
# ---------------------------------------------------------------------------------------------------------------------------
# A close camera inside a wide cloud: Gaussians on both sides of the 1.3 x tanfov clamp, behind the near plane and just in front
SCENE_A = dict(P=160, H=48, W=48, seed=7, sh_degree=1, cam=(10.0, 40.0, 0.9, 50.0),
               scene_kw=dict(radius=1.2, scale_lo=0.05, scale_hi=0.25))
# the same with translucent Gaussians (the alpha image stays below 0.98: T_final = 1 - alpha is well conditioned) and a modifier
SCENE_B = dict(P=200, H=40, W=56, seed=11, sh_degree=2, cam=(25.0, 130.0, 0.8, 45.0), scale_modifier=1.5,
               scene_kw=dict(radius=1.2, scale_lo=0.05, scale_hi=0.25, opa_lo=0.02, opa_hi=0.3))
# floors: half of the populations counted when the scenes were chosen (A: 48 / 34 / 24, B: 98 / 82 / 30); rounding the inputs
# to float32 may move a Gaussian across a threshold but cannot empty a population at these floors
FLOORS = {"A": (24, 17, 12), "B": (49, 41, 15)}
SCENE_MOD = dict(P=120, H=48, W=40, seed=3, sh_degree=1, scene_kw=dict(opa_lo=0.02, opa_hi=0.3))
SCENE_SUBSETS = dict(P=100, H=40, W=56, seed=5, sh_degree=2)
SUBSETS = [("color",), ("depth",), ("alpha",), ("color", "depth"), ("color", "alpha"), ("depth", "alpha"), UPSTREAM]


def _populations(run, cam, H, W, ref_grads):
    """(clamped and visible, those with a non-zero reference gradient, behind the near plane), from the float32 inputs the
    oracle receives."""
    sc, radii = run[0], run[7][1]
    view, _, _, tanx, tany = look_at_camera(cam[0], cam[1], cam[2], cam[3], H, W)
    clamped, behind = clamp_cull_masks(sc["means3D"].numpy(), view.numpy(), tanx, tany)
    vis = clamped & (radii > 0)
    live = vis & (np.abs(ref_grads["means3D"]).max(1) > 0)
    assert not radii[behind].any()
    return (int(vis.sum()), int(live.sum()), int(behind.sum())), behind


def _forward_compare(run):
    sc, leaves, m2d, _, _, out, ro, (color, radii, depth, alpha) = run
    assert np.array_equal(radii, out["radii"].numpy())
    assert np.array_equal(ro.binning()[3].astype(np.int64), out["tiles_touched"].numpy())
    np.testing.assert_allclose(color, out["color"].detach().numpy(), atol=2e-5)
    np.testing.assert_allclose(depth, out["depth"].detach().numpy(), atol=2e-5)
    np.testing.assert_allclose(alpha, out["alpha"].detach().numpy(), atol=2e-5)


@pytest.mark.parametrize("name", ["A", "B"])
def test_clamped_and_culled_gaussians_match_the_fork_clamp_model(oracle, name):
    """The oracle on Gaussians whose Jacobian is clamped (its x / y gradient multipliers) and on culled ones, against the dense
    model that differentiates the clamp as the fork does.  Measured: worst tensor 9e-6 (A), 7e-6 (B) of its maximum."""
    kw = dict(SCENE_A if name == "A" else SCENE_B)
    run = _run(oracle, fork_clamp=True, **kw)
    _forward_compare(run)
    errs, ref = _grad_compare(run, scale_modifier=kw.get("scale_modifier", 1.0))
    pops, behind = _populations(run, kw["cam"], kw["H"], kw["W"], ref)
    print("scene %s: clamped and visible %d, with a gradient %d, behind the near plane %d" % ((name,) + pops))
    assert all(p >= f for p, f in zip(pops, FLOORS[name])), (pops, FLOORS[name])
    if name == "B":
        assert float(run[7][3].max()) < 0.99, "the alpha image must stay away from saturation"
    go = run[6].backward(*(np.ones_like(a) for a in (run[7][0], run[7][2], run[7][3])))
    for k in ref:                           # a culled Gaussian gets exact zeros from both models
        assert not go[k][behind].any() and not ref[k][behind].any(), k


def test_the_clamp_branch_is_not_plain_autograd(oracle):
    """The fork's derivative on the clamped side is a quirk, and scene A reaches it: against plain autograd the oracle's
    dL/dmeans3D is off by tens of per cent (measured 29 % of the maximum).  A scene that stopped reaching the clamp would pass
    the 2e-3 bar here and fail this test."""
    run = _run(oracle, fork_clamp=False, **SCENE_A)
    _forward_compare(run)
    errs, ref = _grad_errors(run)
    print("plain autograd on scene A: %s" % " ".join("%s %.1e" % kv for kv in errs.items()))
    pops, _ = _populations(run, SCENE_A["cam"], SCENE_A["H"], SCENE_A["W"], ref)
    assert all(p >= f for p, f in zip(pops, FLOORS["A"])), (pops, FLOORS["A"])
    assert errs["means3D"] > 0.05, errs
    # the quirk is confined to dL/dmeans3D: every other tensor does not see the clamp's derivative
    assert all(e < GRAD_RTOL for k, e in errs.items() if k != "means3D"), errs


@pytest.mark.parametrize("modifier", [0.5, 2.5])
def test_scale_modifier(oracle, modifier):
    """scale_modifier != 1 on a translucent scene (at 2.5 an opaque one saturates at alpha 0.9999 and the comparison would
    measure the conditioning of T_final = 1 - alpha): radii and tiles_touched exact, images, every gradient, and the scale
    gradient in the fork's convention (oracle * modifier == dense, see _grad_errors).  Measured: worst tensor 2.4e-6 (0.5), 4.5e-6 (2.5)."""
    run = _run(oracle, scale_modifier=modifier, **SCENE_MOD)
    _forward_compare(run)
    assert float(run[7][3].max()) < 0.999 and int((run[7][1] > 0).sum()) >= 100
    errs, ref = _grad_compare(run, scale_modifier=modifier)
    # the convention is visible at this bar: without the factor the scale gradient is off by |1 - 1 / modifier| of its size
    assert _grad_errors(run, scale_modifier=1.0)[0]["scales"] > 0.5


@pytest.mark.parametrize("upstream", SUBSETS, ids=["+".join(s) for s in SUBSETS])
def test_upstream_gradient_subsets(oracle, upstream):
    """Every non-empty subset of (colour, depth, alpha) as the upstream gradients; an absent one is None (a NULL pointer in the
    oracle's backward).  Measured: worst tensor 2.2e-6."""
    run = _run(oracle, **SCENE_SUBSETS)
    errs, ref = _grad_compare(run, upstream=upstream)
    assert np.abs(ref["means3D"]).max() > 0 and np.abs(ref["opacities"]).max() > 0
    if "color" not in upstream:
        assert not ref["shs"].any()         # the colour gradient has no other source: both models must give exact zeros


@pytest.mark.parametrize("H,W", [(3, 5), (8, 9), (17, 33)])
def test_images_smaller_than_a_tile(oracle, H, W):
    """Tiles that lie mostly (17 x 33: a tile row of one pixel row) outside the image.  Measured: worst tensor 6e-5 at 3 x 5."""
    run = _run(oracle, P=40, H=H, W=W, seed=9, sh_degree=1)
    _forward_compare(run)
    assert int((run[7][1] > 0).sum()) >= 20
    _grad_compare(run)


def test_argument_validation(oracle):
    ro = oracle.RasterOracle()
    sc = random_scene(8, 0)
    view, proj, campos, tanx, tany = look_at_camera(0, 0, 2.0, 60, 16, 16)
    with pytest.raises(ValueError):
        ro.forward(image_height=16, image_width=16, tanfovx=tanx, tanfovy=tany, bg=np.zeros(3), scale_modifier=1.0,
                   viewmatrix=view.numpy(), projmatrix=proj.numpy(), sh_degree=0, campos=campos.numpy(),
                   means3D=sc["means3D"].numpy(), opacities=sc["opacities"].numpy(), scales=sc["scales"].numpy(),
                   rotations=sc["rotations"].numpy())  # neither shs nor colors_precomp
