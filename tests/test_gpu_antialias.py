"""GPU tests of the antialiasing mode (GaussianRasterizationSettings.antialiasing: Mip-Splatting's 2-D filter with opacity
compensation) through every layer: kernels (preprocess.hip, gather_backward.hip), C-ABI, Python surface, render().

References: the dense float64 model with opacities * comp (tests/dense_reference.py + tests/antialias_reference.py) on small
scenes; the composite oracle reference (oracle on the compensated opacities, its backward chained through comp; pinned to the
dense model by tests/test_antialias_cpu.py) at the headline size, with the headline bars of test_gpu_headline_parity.py."""
from argparse import ArgumentParser

import numpy as np
import pytest
import torch

import scenes
from antialias_reference import composite_grads, compensation, effective_opacities, scene_compensation
from dense_reference import _quat_to_rot, dense_render
from test_gpu_headline_parity import MAX_LOOSE_ENTRIES, _compare, _upstream
from test_gpu_raster_parity import (_assert_images, _dev, _oracle_forward, _settings, compare_tile_lists,
                                    exact_tile_lists)

pytestmark = pytest.mark.gpu

GRAD_TOL = 2e-3          # max-normalised, the small-size bar of test_gpu_raster_parity.py / test_oracle_vs_dense.py
# the position gradients (means2D and means3D, which takes means2D's term through the projection) against the float64 dense
# model: the float32 kernels sum a few hundred blended entries per pixel at these sizes; measured 2.08e-3 / 2.04e-3 on the
# first scene below.  Every gradient is also held to GRAD_TOL against the float32 composite oracle reference.
DENSE_MEANS_TOL = 3e-3


def _aa(st, on=True):
    return st._replace(antialiasing=on)


def _cov_of(sc):
    R = _quat_to_rot(torch.from_numpy(sc["rotations"]).double())
    L = R * torch.from_numpy(sc["scales"]).double()[:, None, :]
    S = L @ L.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], dim=1).numpy().astype(np.float32)


def _inputs(sc, precomp, seed):
    """numpy inputs of one call: (shs or colors_precomp) and (scales + rotations or cov3D_precomp)."""
    d = dict(means3D=sc["means3D"], opacities=sc["opacities"])
    if precomp:
        d["colors_precomp"] = np.random.default_rng(seed).uniform(0, 1, (sc["means3D"].shape[0], 3)).astype(np.float32)
        d["cov3D_precomp"] = _cov_of(sc)
    else:
        d.update(shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"])
    return d


def _gpu(inp, sts, grads=None, requires_grad=True):
    """One launch set through rasterize_views; with `grads` (gC, gD, gA numpy [V,...]) also the backward.
    Returns (outputs, {input: grad}, means2D grad)."""
    from gaussianip_amd import rasterize_views
    t = {k: _dev(v).requires_grad_(requires_grad) for k, v in inp.items()}
    V, P = len(sts), inp["means3D"].shape[0]
    m2 = torch.zeros(V, P, 3, device="cuda", requires_grad=requires_grad)
    kw = {k: t[k] for k in ("shs", "colors_precomp", "scales", "rotations", "cov3D_precomp") if k in t}
    out = rasterize_views(t["means3D"], m2, t["opacities"], sts, **kw)
    if grads is None:
        return out, None, None
    color, radii, depth, alpha = out
    gC, gD, gA = (_dev(g) for g in grads)
    ((color * gC).sum() + (depth * gD).sum() + (alpha * gA).sum()).backward()
    torch.cuda.synchronize()
    return out, {k: v.grad for k, v in t.items()}, m2.grad


# ------------------------------------------------------------------------------------------------------------------------
# small scenes against the dense float64 antialiased model
# ------------------------------------------------------------------------------------------------------------------------
SMALL = [("stress", 1500, 64, 64, 3, 0, False), ("stress", 2000, 80, 72, 4, 1, False), ("ball", 1500, 64, 64, 5, 2, False),
         ("stress", 1800, 64, 80, 6, 3, False), ("stress", 1600, 72, 64, 8, 0, True)]


@pytest.mark.parametrize("kind,P,H,W,seed,deg,precomp", SMALL)
def test_small_scenes_against_the_dense_antialiased_model(oracle, kind, P, H, W, seed, deg, precomp):
    sc = scenes.make_scene(kind, P, seed=seed, sh_degree=deg)
    cam = scenes.camera(5.0, 90.0, 1.8, 70.0, H, W)
    bg = (0.2, 0.4, 0.1)
    inp = _inputs(sc, precomp, seed)
    rng = np.random.default_rng(seed)
    ups = tuple(rng.normal(size=(1, c, H, W)).astype(np.float32) for c in (3, 1, 1))
    st = _settings(cam, H, W, bg, deg)
    (color, radii, depth, alpha), g, g2d = _gpu(inp, [_aa(st)], ups)
    with torch.no_grad():
        radii_off = _gpu(inp, [st], requires_grad=False)[0][1]
    assert torch.equal(radii, radii_off), "radii must not depend on the flag"
    # dense float64 model, opacity * comp
    leaves = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in inp.items()}
    camd = {k: torch.from_numpy(cam[k]).double() for k in ("viewmatrix", "projmatrix", "campos")}
    cov_kw = {k: leaves[k] for k in ("scales", "rotations", "cov3D_precomp") if k in leaves}
    comp = compensation(means3D=leaves["means3D"], viewmatrix=camd["viewmatrix"], H=H, W=W, tanfovx=cam["tanfovx"],
                        tanfovy=cam["tanfovy"], **cov_kw)
    assert float(comp.min()) < 0.9, "the scene must exercise the compensation"
    m2d = torch.zeros(P, 3, dtype=torch.float64, requires_grad=True)
    out = dense_render(means3D=leaves["means3D"], opacities=leaves["opacities"] * comp[:, None], bg=torch.tensor(bg, dtype=torch.float64),
                       H=H, W=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], sh_degree=deg, means2D=m2d,
                       shs=leaves.get("shs"), colors_precomp=leaves.get("colors_precomp"), **cov_kw, **camd)
    assert np.array_equal(radii[0].cpu().numpy(), out["radii"].numpy())
    for name, ours, ref in (("color", color[0], out["color"]), ("depth", depth[0], out["depth"]), ("alpha", alpha[0], out["alpha"])):
        err = np.abs(ours.detach().cpu().numpy() - ref.detach().numpy())
        # float32 against float64: a pixel where a threshold test (alpha >= 1/255, T < 1e-4) sits within rounding of flipping
        # may decide differently; at most a handful of such entries
        assert int((err > 1e-4).sum()) <= 4 and float(err.max()) < 2e-2, (name, int((err > 1e-4).sum()), float(err.max()))
    upd = [torch.from_numpy(u[0]).double() for u in ups]
    ((out["color"] * upd[0]).sum() + (out["depth"] * upd[1]).sum() + (out["alpha"] * upd[2]).sum()).backward()
    knife, go = _knife_edge_rows(oracle, sc, inp, cam, H, W, bg, deg, ups, alpha[0].detach().cpu().numpy())
    floor = float((leaves["scales"].grad * leaves["scales"]).abs().max()) if "scales" in leaves else 0.0
    for ref_name, checks in (("dense", [("means2D", g2d[0, :, :2], m2d.grad[:, :2].numpy())] + [(k, g[k], leaves[k].grad.numpy()) for k in inp]),
                             ("composite oracle", [("means2D", g2d[0, :, :2], go["means2D"][:, :2])] + [(k, g[k], go[k]) for k in inp])):
        for name, ours, ref in checks:
            err = np.abs(ours.detach().cpu().numpy().reshape(ref.shape) - ref)
            err[knife] = 0.0
            # rotations: an isotropic splat's rotation gradient is analytically 0 -> normalised by the scale gradient's size
            err = err.max() / (max(np.abs(ref).max(), floor if name == "rotations" else 0.0) + 1e-20)
            tol = DENSE_MEANS_TOL if ref_name == "dense" and name in ("means2D", "means3D") else GRAD_TOL
            assert err < tol, "%s against %s: max error / max |grad| = %.3e" % (name, ref_name, err)


def _knife_edge_rows(oracle, sc, inp, cam, H, W, bg, deg, ups, alpha_np):
    """(rows to leave out, composite oracle gradients).  Gaussians that take part in a PROVEN knife-edge pixel (oracle.knife_edge_gaussians: a threshold test of the blend within
    2e-5 of flipping), found by the oracle on the compensated opacities.  The kernels compute comp in float32, the references in
    float64, so such a test may decide differently and move that Gaussian's gradient by a whole pixel contribution; these rows
    are left out of the gradient bars here (measured at 100k / 1024^2: one Gaussian, 2.7e-3 of the maximum, every other row
    within 4e-5)."""
    comp, _ = scene_compensation(sc, cam, H, W, cov=inp.get("cov3D_precomp"))
    kw = dict(colors=inp.get("colors_precomp"), cov=inp.get("cov3D_precomp"))
    ro, _ = _oracle_forward(oracle, dict(sc, opacities=effective_opacities(sc, comp)), cam, H, W, bg, deg, **kw)
    go = ro.backward(ups[0][0], ups[1][0], ups[2][0], alpha_out=alpha_np)
    return ro.knife_edge_gaussians()[0], composite_grads(go, sc, cam, H, W, cov=inp.get("cov3D_precomp"))


# ------------------------------------------------------------------------------------------------------------------------
# tile / index buffers
# ------------------------------------------------------------------------------------------------------------------------
def _state(inp, st):
    from gaussianip_amd import rasterizer as R
    kw = {k: _dev(v) for k, v in inp.items() if k not in ("means3D", "opacities")}
    outs, plan = R.forward_with_state(_dev(inp["means3D"]), _dev(inp["opacities"]), [st], **kw)
    torch.cuda.synchronize()
    return outs, plan, R.state_views(plan)


def test_tile_lists_with_the_flag(oracle, monkeypatch):
    """Exact lists: the tile / index buffers do not depend on opacity, so they are bit-identical with the flag on and off, and
    the oracle's on the compensated opacities; n_contrib matches that oracle run.  Default lists: only tiles the compensated
    alpha >= 1/255 region reaches get an instance (no more than without the flag), each dropped entry is provably dead, and
    the images are those of the exact lists."""
    P, H, W, deg, bg = 3000, 96, 112, 1, (0.0, 0.0, 0.0)
    sc = scenes.make_scene("stress", P, seed=12, sh_degree=deg)
    cam = scenes.camera(5.0, 90.0, 1.8, 70.0, H, W)
    inp = _inputs(sc, False, 0)
    st = _settings(cam, H, W, bg, deg)
    comp, _ = scene_compensation(sc, cam, H, W)
    ro, (o_color, o_radii, o_depth, o_alpha) = _oracle_forward(oracle, dict(sc, opacities=effective_opacities(sc, comp)), cam, H, W, bg, deg)
    keys, vals, ranges, tt, nc = ro.binning()
    res = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("GIP_RASTER_EXACT_LISTS", mode)
        for on in (False, True):
            res[mode, on] = _state(inp, _aa(st, on))
    monkeypatch.delenv("GIP_RASTER_EXACT_LISTS")
    (c_off, r_off, _, _), _, sv_off = res["1", False]
    (color, radii, depth, alpha), _, sv = res["1", True]
    n = int(sv["header"][1])
    assert n == int(sv_off["header"][1])
    assert torch.equal(sv["keys"][:n], sv_off["keys"][:n]), "sorted key / value lists"
    assert torch.equal(sv["tile_start"], sv_off["tile_start"]), "ranges"
    assert torch.equal(sv["records_u32"][0][:, 7], sv_off["records_u32"][0][:, 7]), "tiles_touched"
    assert torch.equal(sv["records_u32"][0][:, 12:14], sv_off["records_u32"][0][:, 12:14]), "rectangles"
    assert torch.equal(radii, r_off) and np.array_equal(radii[0].cpu().numpy(), o_radii)
    assert not torch.equal(color, c_off)
    exact_tile_lists(sv, sv["header"].cpu().numpy(), keys, vals, ranges, tt)
    _assert_images(ro, color[0], depth[0], alpha[0], o_color, o_depth, o_alpha, sv["n_contrib"][0], nc)
    # default lists
    (dc, dr, dd, da), _, dsv = res["0", True]
    n_on, n_off = int(dsv["header"][1]), int(res["0", False][2]["header"][1])
    print("num_rendered (default lists): flag off %d, flag on %d; exact lists %d" % (n_off, n_on, n))
    assert n_on <= n_off
    nc_expected = compare_tile_lists(dsv, dsv["header"].cpu().numpy(), ro.geom(), keys, vals, ranges, tt, nc, H, W, min_keep=0.1)
    _assert_images(ro, dc[0], dd[0], da[0], o_color, o_depth, o_alpha, dsv["n_contrib"][0], nc_expected)
    assert torch.equal(dr, radii)
    for a, b in ((dc, color), (dd, depth), (da, alpha)):
        assert float((a - b).abs().max()) < 5e-6 * max(1.0, float(b.abs().max()))


# ------------------------------------------------------------------------------------------------------------------------
# 100 000 Gaussians at 1024^2 against the composite oracle reference, headline bars
# ------------------------------------------------------------------------------------------------------------------------
HP, HH, HW = 100000, 1024, 1024
_oracle_cache = {}


def _headline_scene(look, deg):
    sc = scenes.make_scene("human", HP, seed=42, sh_degree=deg)
    if look == "trained":
        scenes.trained_look(sc, seed=7)
    if deg > 0:
        sc["shs"][:, 1:, :] = np.random.default_rng(3).normal(size=(HP, (deg + 1) ** 2 - 1, 3)).astype(np.float32) * 0.1
    return sc


def _composite_reference(oracle, sc, cams, bg, deg, ups, alpha_np):
    """Per view: oracle images / radii on the compensated opacities, its backward on the GPU's alpha image chained
    through comp, and the knife-edge classes of test_gpu_headline_parity._compare."""
    oracle.set_threads(oracle.max_threads())
    try:
        res = []
        for v, cam in enumerate(cams):
            comp, _ = scene_compensation(sc, cam, HH, HW)
            ro, out = _oracle_forward(oracle, dict(sc, opacities=effective_opacities(sc, comp)), cam, HH, HW, bg, deg)
            go = ro.backward(ups[0][v], ups[1][v], ups[2][v], alpha_out=alpha_np[v])
            knife, _, behind = ro.knife_edge_gaussians(sharing=True)
            res.append(dict(ro=ro, out=out, grads=composite_grads(go, sc, cam, HH, HW), knife=knife, behind=behind,
                            num_rendered=ro.num_rendered))
    finally:
        oracle.set_threads(1)
    return res


def _settled(ours, ref, knife):
    """`ours` with the rows of proven knife-edge Gaussians replaced by the reference: see _knife_edge_rows."""
    ours = ours.detach().cpu().numpy().reshape(ref.shape).astype(np.float64)
    ours[knife] = ref[knife]
    return torch.from_numpy(ours)


def _check_headline(tag, sc, inp, out, g, g2d, ref):
    color, radii, depth, alpha = out
    for v, r in enumerate(ref):
        o_color, o_radii, o_depth, o_alpha = r["out"]
        assert np.array_equal(radii[v].cpu().numpy(), o_radii), "radii of view %d" % v
        _assert_images(r["ro"], color[v], depth[v], alpha[v], o_color, o_depth, o_alpha)
        print("%s view %d: %d knife-edge Gaussians" % (tag, v, int(r["knife"].sum())))
        _compare(tag, "means2D[%d]" % v, _settled(g2d[v], r["grads"]["means2D"], r["knife"]), r["grads"]["means2D"],
                 skip_rows=r["knife"], loose_rows=r["behind"])
    knife = np.logical_or.reduce([r["knife"] for r in ref])
    behind = np.logical_or.reduce([r["behind"] for r in ref])
    tot = {k: sum(r["grads"][k] for r in ref) for k in inp if k != "means2D"}
    rot_floor = float(np.abs(tot["scales"] * sc["scales"]).max())
    M = sc["shs"].shape[1]
    for k in ("means3D", "opacities", "shs", "scales", "rotations"):
        # the loose-entry allowance counts entries: a Gaussian has 3 M of them in dL/dshs (M = 1 where it was measured)
        _compare(tag, k, _settled(g[k], tot[k], knife), tot[k], floor=rot_floor if k == "rotations" else 0.0, skip_rows=knife,
                 loose_rows=behind, max_loose=MAX_LOOSE_ENTRIES * (M if k == "shs" else 1))


@pytest.mark.parametrize("look", ["init", "trained"])
def test_single_view_at_100k_1024_against_the_composite_reference(oracle, look):
    sc = _headline_scene(look, 0)
    cams = scenes.train_cameras(4, 42, HH, HW)[:1]
    bg = (0.0, 0.0, 0.0) if look == "init" else (0.2, 0.4, 0.1)
    inp = _inputs(sc, False, 0)
    ups = _upstream(3)
    out, g, g2d = _gpu(inp, [_aa(_settings(c, HH, HW, bg, 0)) for c in cams], ups)
    ref = _composite_reference(oracle, sc, cams, bg, 0, ups, out[3].detach().cpu().numpy())
    _check_headline("antialiasing 1 view / " + look, sc, inp, out, g, g2d, ref)


@pytest.mark.parametrize("sh_path", ["matrix cores", "scalar"])
def test_four_view_launch_set_at_100k_1024_sh3_against_the_composite_reference(oracle, monkeypatch, sh_path):
    monkeypatch.setenv("GIP_RASTER_SH_SCALAR", "1" if sh_path == "scalar" else "0")
    deg, bg = 3, (0.0, 0.0, 0.0)
    sc = _headline_scene("init", deg)
    cams = scenes.train_cameras(4, 42, HH, HW)
    inp = _inputs(sc, False, 0)
    ups = _upstream(5, V=4)
    out, g, g2d = _gpu(inp, [_aa(_settings(c, HH, HW, bg, deg)) for c in cams], ups)
    if "ref" not in _oracle_cache:         # both SH paths against one reference (the backward sees the first path's alpha image)
        _oracle_cache["ref"] = _composite_reference(oracle, sc, cams, bg, deg, ups, out[3].detach().cpu().numpy())
    _check_headline("antialiasing 4 views sh3 / " + sh_path, sc, inp, out, g, g2d, _oracle_cache["ref"])


# ------------------------------------------------------------------------------------------------------------------------
# launch sets, determinism, forward-only, argument checks
# ------------------------------------------------------------------------------------------------------------------------
def test_launch_set_equals_per_view_calls(monkeypatch):
    from gaussianip_amd import GaussianRasterizer
    monkeypatch.setenv("GIP_RASTER_SH_SCALAR", "1")
    P, H, W = 4000, 96, 128
    sc = scenes.make_scene("stress", P, seed=5, sh_degree=1)
    cams = scenes.train_cameras(4, 9, H, W)
    sts = [_aa(_settings(c, H, W, (0.0, 0.0, 0.0), 1)) for c in cams]
    inp = _inputs(sc, False, 0)
    rng = np.random.default_rng(1)
    ups = tuple(rng.normal(size=(4, c, H, W)).astype(np.float32) for c in (3, 1, 1))
    (color, radii, depth, alpha), batched, m2g = _gpu(inp, sts, ups)
    t = {k: _dev(v).requires_grad_(True) for k, v in inp.items()}
    for i, s in enumerate(sts):
        m = torch.zeros(P, 3, device="cuda", requires_grad=True)
        c1, r1, d1, a1 = GaussianRasterizer(s)(means3D=t["means3D"], means2D=m, opacities=t["opacities"], shs=t["shs"],
                                               scales=t["scales"], rotations=t["rotations"])
        assert torch.equal(c1, color[i]) and torch.equal(d1, depth[i]) and torch.equal(a1, alpha[i]) and torch.equal(r1, radii[i])
        ((c1 * _dev(ups[0][i])).sum() + (d1 * _dev(ups[1][i])).sum() + (a1 * _dev(ups[2][i])).sum()).backward()
        assert torch.equal(m.grad, m2g[i])
    for k in t:
        ref = t[k].grad
        assert float((batched[k] - ref).abs().max() / (ref.abs().max() + 1e-20)) < 1e-5, k


def test_backward_is_bitwise_reproducible_and_no_grad_forward_is_bit_identical():
    P, H, W = 3000, 96, 96
    sc = scenes.make_scene("stress", P, seed=31, sh_degree=1)
    cams = scenes.train_cameras(2, 6, H, W)
    sts = [_aa(_settings(c, H, W, (0.1, 0.2, 0.3), 1)) for c in cams]
    inp = _inputs(sc, False, 0)
    rng = np.random.default_rng(2)
    ups = tuple(rng.normal(size=(2, c, H, W)).astype(np.float32) for c in (3, 1, 1))
    a_out, a, a2 = _gpu(inp, sts, ups)
    b_out, b, b2 = _gpu(inp, sts, ups)
    assert torch.equal(a2, b2) and all(torch.equal(a[k], b[k]) for k in a)
    with torch.no_grad():
        f_out = _gpu(inp, sts, requires_grad=False)[0]
    for x, y, z in zip(a_out, b_out, f_out):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_launch_set_mixing_the_flag_is_rejected():
    from gaussianip_amd import rasterize_views
    P, H, W = 500, 32, 32
    sc = scenes.make_scene("ball", P, seed=1)
    cams = scenes.train_cameras(2, 1, H, W)
    sts = [_settings(cams[0], H, W, (0.0, 0.0, 0.0), 0), _aa(_settings(cams[1], H, W, (0.0, 0.0, 0.0), 0))]
    t = {k: _dev(v) for k, v in sc.items()}
    with pytest.raises(ValueError, match="antialiasing"):
        rasterize_views(t["means3D"], None, t["opacities"], sts, shs=t["shs"], scales=t["scales"], rotations=t["rotations"])


# ------------------------------------------------------------------------------------------------------------------------
# render() / render_views() through PipelineParams
# ------------------------------------------------------------------------------------------------------------------------
def _model_and_cameras():
    from test_gpu_pipeline import _camera, _model
    return _model(P=4000, seed=11), [_camera(10.0, 30.0 + 90.0 * i, 1.6, 55.0, 128, 112) for i in range(2)]


def _grads(gm, loss, means2D):
    params = [gm._xyz, gm._features_dc, gm._features_rest, gm._scaling, gm._rotation, gm._opacity, means2D]
    return torch.autograd.grad(loss, params, allow_unused=True)


def test_render_and_render_views_take_the_flag_from_pipeline_params():
    from gaussianip_amd import GaussianRasterizer, rasterize_views
    from gaussianip_amd.arguments import PipelineParams
    from gaussianip_amd.renderer import _settings as r_settings
    from gaussianip_amd.renderer import render, render_views
    gm, cams = _model_and_cameras()
    bg = torch.tensor([0.1, 0.2, 0.3], device="cuda")
    on, off = PipelineParams(ArgumentParser(), antialiasing=True), PipelineParams(ArgumentParser())
    p_on, p_off = render(cams[0], gm, on, bg), render(cams[0], gm, off, bg)
    st = r_settings(cams[0], gm, bg, 1.0)
    assert st.antialiasing is False
    direct = GaussianRasterizer(_aa(st))(means3D=gm.get_xyz, means2D=None, opacities=gm.get_opacity, shs=gm.get_features,
                                         scales=gm.get_scaling, rotations=gm.get_rotation)
    assert torch.equal(p_on["render"], direct[0]) and torch.equal(p_on["alpha_3dgs"], direct[3])
    assert torch.equal(p_on["radii"], p_off["radii"]) and not torch.equal(p_on["render"], p_off["render"])
    assert float(p_on["alpha_3dgs"].sum()) < float(p_off["alpha_3dgs"].sum())
    v_on = render_views(cams, gm, on, bg)
    sts = [_aa(r_settings(c, gm, bg, 1.0)) for c in cams]
    o, s, q = gm.get_activated()                    # what render_views takes its activations from
    d_views = rasterize_views(gm.get_xyz, None, o, sts, shs=gm.get_features, scales=s, rotations=q)
    assert torch.equal(v_on["render"], d_views[0]) and torch.equal(v_on["depth_3dgs"], d_views[2])
    v_off = render_views(cams, gm, off, bg)
    assert not torch.equal(v_on["render"], v_off["render"])


def test_explicit_false_is_bit_identical_to_settings_without_the_field():
    from gaussianip_amd import GaussianRasterizationSettings, GaussianRasterizer
    from gaussianip_amd.renderer import _settings as r_settings
    gm, cams = _model_and_cameras()
    bg = torch.tensor([0.1, 0.2, 0.3], device="cuda")
    st = r_settings(cams[0], gm, bg, 1.0)
    fork = GaussianRasterizationSettings(*st[:12])                  # the fork's 12 fields
    explicit = fork._replace(antialiasing=False)
    res = []
    for s in (fork, explicit):
        m2 = torch.zeros_like(gm.get_xyz, requires_grad=True)
        out = GaussianRasterizer(s)(means3D=gm.get_xyz, means2D=m2, opacities=gm.get_opacity, shs=gm.get_features,
                                    scales=gm.get_scaling, rotations=gm.get_rotation)
        loss = out[0].square().mean() + out[2].mean() + out[3].mean()
        res.append((out, _grads(gm, loss, m2)))
    for x, y in zip(res[0][0], res[1][0]):
        assert torch.equal(x, y)
    for x, y in zip(res[0][1], res[1][1]):
        assert (x is None and y is None) or torch.equal(x, y)


def test_render_deformed_takes_the_flag_as_a_keyword():
    from gaussianip_amd.renderer import render_deformed
    gm, cams = _model_and_cameras()
    bg = torch.tensor([0.0, 0.0, 0.0], device="cuda")
    args = (cams[0], gm.get_xyz, gm.get_opacity, gm.get_scaling, gm.get_rotation, gm.get_features, gm.active_sh_degree, bg)
    with torch.no_grad():
        off, default, on = render_deformed(*args, antialiasing=False), render_deformed(*args), render_deformed(*args, antialiasing=True)
    assert torch.equal(off["render"], default["render"]) and torch.equal(on["radii"], off["radii"])
    assert not torch.equal(on["render"], off["render"])
