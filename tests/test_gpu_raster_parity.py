"""GPU parity: the HIP rasterizer, called through the C-ABI (ctypes), against the CPU oracle on identical inputs.

Bars: tile / index buffers bit-exact; RGB / depth / alpha within 1e-4; gradients within 2e-3 of the
largest gradient magnitude per tensor (the CUDA reference itself sums float atomics in arbitrary order)."""
import os

import numpy as np
import pytest
import torch

import scenes

pytestmark = pytest.mark.gpu

IMG_TOL = 1e-4
BACKWARD_TOL = 2e-3          # of the largest gradient magnitude per tensor


def _settings(cam, H, W, bg, sh_degree, scale_modifier=1.0):
    from gaussianip_amd import GaussianRasterizationSettings
    dev = "cuda"
    return GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
        bg=torch.tensor(bg, dtype=torch.float32, device=dev), scale_modifier=scale_modifier,
        viewmatrix=torch.from_numpy(cam["viewmatrix"]).to(dev), projmatrix=torch.from_numpy(cam["projmatrix"]).to(dev),
        sh_degree=sh_degree, campos=torch.from_numpy(cam["campos"]).to(dev), prefiltered=False, debug=False)


def _oracle_forward(oracle, sc, cam, H, W, bg, sh_degree, scale_modifier=1.0, colors=None, cov=None):
    ro = oracle.RasterOracle()
    kw = dict(image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=np.asarray(bg, np.float32),
              scale_modifier=scale_modifier, viewmatrix=cam["viewmatrix"], projmatrix=cam["projmatrix"],
              sh_degree=sh_degree, campos=cam["campos"], means3D=sc["means3D"], opacities=sc["opacities"])
    if colors is None:
        kw["shs"] = sc["shs"]
    else:
        kw["colors_precomp"] = colors
    if cov is None:
        kw.update(scales=sc["scales"], rotations=sc["rotations"])
    else:
        kw["cov3D_precomp"] = cov
    out = ro.forward(**kw)
    return ro, out


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_forward(oracle, kind, P, H, W, seed, sh_degree, cam_args, bg=(0.0, 0.0, 0.0), nc_mismatch_frac=2e-4):
    sc = scenes.make_scene(kind, P, seed=seed, sh_degree=sh_degree)
    cam = scenes.camera(*cam_args, H, W)
    return _check_forward_scene(oracle, sc, cam, H, W, sh_degree, bg, nc_mismatch_frac)[0]


def _check_forward_scene(oracle, sc, cam, H, W, sh_degree, bg=(0.0, 0.0, 0.0), nc_mismatch_frac=2e-4, min_keep=0.5, stats=None,
                         scale_modifier=1.0, outputs=None):
    """Forward of one view through the C-ABI against the oracle: integer buffers bit-exact, images within IMG_TOL.
    Returns (num_rendered, oracle object with its forward state) so a backward comparison can follow.
    `stats`: a dict that receives the library's header words and the number of (proven knife-edge) pixels out of tolerance.
    `outputs`: a dict that receives the images, the radii and the plan of the call."""
    from gaussianip_amd import rasterizer as R
    ro, (o_color, o_radii, o_depth, o_alpha) = _oracle_forward(oracle, sc, cam, H, W, bg, sh_degree, scale_modifier)
    st = _settings(cam, H, W, bg, sh_degree, scale_modifier)
    (color, radii, depth, alpha), plan = R.forward_with_state(
        _dev(sc["means3D"]), _dev(sc["opacities"]), [st], shs=_dev(sc["shs"]), scales=_dev(sc["scales"]),
        rotations=_dev(sc["rotations"]))
    torch.cuda.synchronize()
    sv = R.state_views(plan)
    Rn = ro.num_rendered
    # ---- integer buffers: bit-exact ----
    assert np.array_equal(radii[0].cpu().numpy(), o_radii), "radii"
    keys, vals, ranges, tt, nc = ro.binning()
    hdr = sv["header"].cpu().numpy()
    geom = ro.geom()
    rec_f = sv["records"][0].cpu().numpy()
    vis = o_radii > 0
    assert np.array_equal(rec_f[vis, 0:2].view(np.uint32), geom["means2D"][vis].view(np.uint32)), "means2D bits"
    assert np.array_equal(rec_f[vis, 2].view(np.uint32), geom["depths"][vis].view(np.uint32)), "depth bits"
    assert np.array_equal(rec_f[vis, 4:7].view(np.uint32), geom["conic_opacity"][vis, :3].view(np.uint32)), "conic bits"
    assert np.array_equal(rec_f[vis, 8:11].view(np.uint32), geom["rgb"][vis].view(np.uint32)), "rgb bits"
    if os.environ.get("GIP_RASTER_EXACT_LISTS", "0") == "1":
        exact_tile_lists(sv, hdr, keys, vals, ranges, tt)
        nc_expected = nc
    else:
        nc_expected = compare_tile_lists(sv, hdr, geom, keys, vals, ranges, tt, nc, H, W, min_keep=min_keep)
    # ---- images ----
    n_out = _assert_images(ro, color[0], depth[0], alpha[0], o_color, o_depth, o_alpha, sv["n_contrib"][0], nc_expected,
                           nc_mismatch_frac)
    if outputs is not None:
        outputs.update(color=color, radii=radii, depth=depth, alpha=alpha, plan=plan)
    if stats is not None:
        ts = sv["tile_start"].cpu().numpy().astype(np.int64)
        stats.update(num_rendered=int(hdr[1]), max_tile_count=int(hdr[3]), num_segments=int(hdr[5]), pixels_out_of_tolerance=n_out,
                     n_contrib_median=float(np.median(sv["n_contrib"][0].cpu().numpy())), lists_median=int(np.median(ts[1:] - ts[:-1])))
    return Rn, ro


def exact_tile_lists(sv, hdr, keys, vals, ranges, tt):
    """GIP_RASTER_EXACT_LISTS=1: tiles_touched, num_rendered, the sorted key / value lists and the tile ranges are the
    oracle's (= the fork's buffers) bit for bit."""
    Rn = len(vals)
    rec_u = sv["records_u32"][0].cpu().numpy()
    assert np.array_equal(rec_u[:, 7].astype(np.uint32), tt), "tiles_touched"
    assert int(hdr[1]) == Rn and int(hdr[2]) == 0, "num_rendered / overflow"
    my_keys = sv["keys"][:Rn].cpu().numpy().view(np.uint64)
    assert np.array_equal((my_keys & np.uint64(0xffffffff)).astype(np.uint32), vals), "point_list"
    assert np.array_equal(my_keys >> np.uint64(32), keys & np.uint64(0xffffffff)), "sorted depth keys"
    ts = sv["tile_start"].cpu().numpy().astype(np.int64)
    cnt = (ranges[:, 1].astype(np.int64) - ranges[:, 0].astype(np.int64))
    assert np.array_equal(ts[1:] - ts[:-1], cnt), "per-tile counts"
    ne = cnt > 0
    assert np.array_equal(ts[:-1][ne], ranges[ne, 0].astype(np.int64)), "ranges.x"
    assert np.array_equal(ts[1:][ne], ranges[ne, 1].astype(np.int64)), "ranges.y"


def compare_tile_lists(sv, hdr, geom, keys, vals, ranges, tt, nc, H, W, min_keep=0.5):
    """The per-tile lists against the oracle's (= the fork's sorted (tile | depth) key / value buffers).  The library makes
    instances only for the tiles the alpha >= 1/255 region of a Gaussian can reach, so its lists are the oracle's lists
    WITHOUT some entries; asserted here, bit-exactly:
      * the kept entries are the oracle's, in the oracle's order (same Gaussian ids, same depth keys, tile by tile);
      * every dropped entry is dead: at no pixel of its tile does it pass the fork's alpha >= 1/255 test (brute force over
        the 256 pixels with the oracle's conic / opacity), and the drop rate is plausible (never more than half);
      * tiles_touched / num_rendered / the ranges are those of the kept lists.
    Returns the oracle's n_contrib image re-expressed as positions in the kept lists."""
    P = tt.shape[0]
    tiles_x = (W + 15) // 16
    T = ranges.shape[0]
    ts = sv["tile_start"].cpu().numpy().astype(np.int64)
    Rg = int(hdr[1])
    assert int(hdr[2]) == 0 and ts[-1] == Rg, "overflow / num_rendered"
    my_keys = sv["keys"][:Rg].cpu().numpy().view(np.uint64)
    g_idx = (my_keys & np.uint64(0xffffffff)).astype(np.int64)
    g_tile = np.repeat(np.arange(T, dtype=np.int64), ts[1:] - ts[:-1])
    o_tile = (keys >> np.uint64(32)).astype(np.int64)
    o_idx = vals.astype(np.int64)
    o_pair, g_pair = o_tile * P + o_idx, g_tile * P + g_idx
    kept = np.isin(o_pair, g_pair)
    assert kept.sum() == Rg and np.array_equal(o_pair[kept], g_pair), "kept entries = the oracle's entries, in its order"
    assert np.array_equal(my_keys >> np.uint64(32), (keys & np.uint64(0xffffffff))[kept]), "sorted depth keys"
    assert Rg >= min_keep * max(len(o_pair), 1), "implausible drop rate"
    rec_u = sv["records_u32"][0].cpu().numpy()
    assert np.array_equal(rec_u[:, 7].astype(np.int64), np.bincount(g_idx, minlength=P)), "tiles_touched of the kept lists"
    # dropped entries are dead (float64 evaluation of the fork's test on every pixel of the tile, no margin needed: the
    # library's bound is conservative by > 1 %)
    dropped = np.flatnonzero(~kept)

    def contributes(d):
        co = geom["conic_opacity"][o_idx[d]].astype(np.float64)
        mx, my = geom["means2D"][o_idx[d], 0].astype(np.float64), geom["means2D"][o_idx[d], 1].astype(np.float64)
        x0, y0 = (o_tile[d] % tiles_x) * 16.0, (o_tile[d] // tiles_x) * 16.0
        off = np.arange(16, dtype=np.float64)
        dx = (mx - x0)[:, None, None] - off[None, None, :]
        dy = (my - y0)[:, None, None] - off[None, :, None]
        power = -0.5 * (co[:, 0, None, None] * dx * dx + co[:, 2, None, None] * dy * dy) - co[:, 1, None, None] * dx * dy
        a = np.minimum(0.99, co[:, 3, None, None] * np.exp(np.minimum(power, 0.0)))
        return bool(((power <= 0) & (a >= 1.0 / 255.0)).any())

    # in blocks of 1024 entries (256 float64 per entry and temporary: a million dropped entries would not fit at once), a few
    # blocks at a time (numpy releases the interpreter lock inside its loops)
    blocks = [dropped[s:s + 1024] for s in range(0, dropped.size, 1024)]
    if len(blocks) > 8:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(4) as pool:
            alive = any(pool.map(contributes, blocks))
    else:
        alive = any(contributes(b) for b in blocks)
    assert not alive, "a dropped instance would have contributed"
    # n_contrib: position of the last contributor, counted in the kept list of its tile
    ck = np.concatenate([[0], np.cumsum(kept)])
    tile_of_pixel = (np.arange(H)[:, None] // 16) * tiles_x + (np.arange(W)[None, :] // 16)
    lo = ranges[tile_of_pixel, 0].astype(np.int64)
    lo = np.where(nc > 0, lo, 0)
    return (ck[lo + nc.astype(np.int64)] - ck[lo]).astype(np.uint32)


KNIFE_EDGE = 2e-5


def _assert_images(ro, color, depth, alpha, o_color, o_depth, o_alpha, n_contrib=None, o_n_contrib=None,
                   max_frac=2e-4):
    """colour / alpha within IMG_TOL, depth within IMG_TOL * max(1, depth), n_contrib equal — at every pixel except
    PROVEN knife-edge pixels: pixels where one of the walk's threshold tests (alpha >= 1/255, T (1 - alpha) >= 1e-4,
    power <= 0) sits within KNIFE_EDGE (relative) of flipping in the oracle, so that libm expf and v_exp_f32 may
    legitimately decide differently (the same holds between the CUDA fork's expf and any CPU statement).  Their number is
    bounded by `max_frac` of the image as well."""
    color, depth, alpha = (t.detach().cpu().numpy() for t in (color, depth, alpha))
    bad = (np.abs(color - o_color) > IMG_TOL).any(0)
    bad |= np.abs(depth[0] - o_depth[0]) > IMG_TOL * max(1.0, float(o_depth.max()))
    bad |= np.abs(alpha[0] - o_alpha[0]) > IMG_TOL
    if n_contrib is not None:
        bad |= n_contrib.cpu().numpy().astype(np.uint32) != o_n_contrib
    ids = np.flatnonzero(bad.reshape(-1))
    assert ids.size <= max_frac * bad.size, "%d pixels out of tolerance" % ids.size
    if ids.size:
        margins = ro.pixel_margins(ids)
        worst = int(np.argmax(margins))
        assert margins[worst] < KNIFE_EDGE, (
            "pixel %d differs from the oracle by more than the tolerance and is NOT a knife-edge pixel (margin %.2e)"
            % (ids[worst], margins[worst]))
    return ids.size


@pytest.mark.parametrize("kind,P,H,W,seed,deg", [
    ("ball", 2000, 64, 64, 1, 0),
    ("stress", 3000, 80, 112, 2, 1),
    ("stress", 1500, 100, 60, 3, 3),
    ("ball", 10000, 256, 256, 42, 0),      # BASELINE.json configs[0]
    ("stress", 10000, 256, 256, 43, 2),
])
def test_forward_parity(oracle, kind, P, H, W, seed, deg):
    R = _check_forward(oracle, kind, P, H, W, seed, deg, (5.0, 90.0, 1.8, 70.0), bg=(0.1, 0.2, 0.3))
    assert R > 0


@pytest.mark.parametrize("kind,P,H,W,seed,deg", [("stress", 3000, 80, 112, 2, 1), ("ball", 10000, 256, 256, 42, 0)])
def test_forward_parity_exact_lists(oracle, monkeypatch, kind, P, H, W, seed, deg):
    """GipRasterConfig::exact_lists (GIP_RASTER_EXACT_LISTS=1): every tile of the fork's 3-sigma rectangle gets its instance —
    tiles_touched, num_rendered, the sorted (depth, index) lists, the ranges and n_contrib equal the oracle's bit for bit,
    and the images are those of the default (culled) mode."""
    from gaussianip_amd import rasterizer as R
    monkeypatch.setenv("GIP_RASTER_EXACT_LISTS", "1")
    Rn = _check_forward(oracle, kind, P, H, W, seed, deg, (5.0, 90.0, 1.8, 70.0), bg=(0.1, 0.2, 0.3))
    sc = scenes.make_scene(kind, P, seed=seed, sh_degree=deg)
    cam = scenes.camera(5.0, 90.0, 1.8, 70.0, H, W)
    st = _settings(cam, H, W, (0.1, 0.2, 0.3), deg)
    args = (_dev(sc["means3D"]), _dev(sc["opacities"]), [st])
    kw = dict(shs=_dev(sc["shs"]), scales=_dev(sc["scales"]), rotations=_dev(sc["rotations"]))
    (c1, r1, d1, a1), p1 = R.forward_with_state(*args, **kw)
    monkeypatch.setenv("GIP_RASTER_EXACT_LISTS", "0")
    (c0, r0, d0, a0), p0 = R.forward_with_state(*args, **kw)
    torch.cuda.synchronize()
    assert int(R.state_views(p1)["header"][1]) == Rn > int(R.state_views(p0)["header"][1])
    assert torch.equal(r0, r1) and float((c0 - c1).abs().max()) < 2e-6 and float((a0 - a1).abs().max()) < 2e-6


def test_forward_parity_close_camera_big_tiles(oracle):
    # camera inside the cloud: huge splats, near-plane culling, long per-tile lists (exercises the 8192 sort class)
    _check_forward(oracle, "stress", 6000, 96, 96, 7, 0, (10.0, 30.0, 0.35, 80.0))


def _max_norm_error(ours, ref, floor=0.0):
    """The figure _check_backward holds to its bar: the largest error over the whole tensor, relative to the tensor's largest
    |gradient| (or `floor`)."""
    scale = max(float(np.abs(ref).max()), floor) + 1e-20
    return np.abs(ours.reshape(ref.shape) - ref).max() / scale


def _check_backward(oracle, kind, P, H, W, seed, sh_degree, use_precomp=False, bg=(0.3, 0.1, 0.2), tol=BACKWARD_TOL, scene=None, cam=None,
                    tol_e2e=5e-3, geom_tol=None, scale_modifier=1.0, upstream=("color", "depth", "alpha"), cov=None, outputs=None):
    """`scale_modifier`: of the settings and of the oracle (both return the scale gradient with respect to modifier * scale).
    `upstream`: the outputs that get an upstream gradient; the others are left out of the loss, so their gradient reaches the
    kernels as a NULL pointer, and go to the oracle as None.  `cov`: the [P,6] covariances of a `use_precomp` call (default: the
    oracle's own).  `outputs`: a dict that receives the images, radii and the gradients of the precomputed inputs."""
    from gaussianip_amd import GaussianRasterizer
    sc = scenes.make_scene(kind, P, seed=seed, sh_degree=sh_degree) if scene is None else scene
    cam = scenes.camera(8.0, 60.0, 1.7, 60.0, H, W) if cam is None else cam
    rng = np.random.default_rng(seed + 100)
    gC = rng.normal(size=(3, H, W)).astype(np.float32)
    gD = rng.normal(size=(1, H, W)).astype(np.float32)
    gA = rng.normal(size=(1, H, W)).astype(np.float32)
    colors = None
    gC, gD, gA = (g if k in upstream else None for k, g in zip(("color", "depth", "alpha"), (gC, gD, gA)))
    if use_precomp:
        colors = rng.uniform(0, 1, (P, 3)).astype(np.float32)
    if use_precomp and cov is None:
        ro0, _ = _oracle_forward(oracle, sc, cam, H, W, bg, sh_degree)
        cov = ro0.geom()["cov3D"]
        bad = ~(np.abs(cov).sum(1) > 0)   # culled Gaussians have no cov3D in the oracle state: rebuild analytically
        if bad.any():
            from dense_reference import _quat_to_rot
            Rm = _quat_to_rot(torch.from_numpy(sc["rotations"]).double())
            L = Rm * torch.from_numpy(sc["scales"]).double()[:, None, :]
            S = (L @ L.transpose(1, 2)).numpy()
            full = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(np.float32)
            cov[bad] = full[bad]
    ro, o_out = _oracle_forward(oracle, sc, cam, H, W, bg, sh_degree, scale_modifier, colors=colors, cov=cov)
    go_e2e = ro.backward(gC, gD, gA)

    st = _settings(cam, H, W, bg, sh_degree, scale_modifier)
    t = {k: _dev(v).requires_grad_(True) for k, v in sc.items()}
    means2D = torch.zeros(P, 3, device="cuda", requires_grad=True)
    kw = dict(means3D=t["means3D"], means2D=means2D, opacities=t["opacities"])
    tc = tv = None
    if use_precomp:
        tc = _dev(colors).requires_grad_(True)
        tv = _dev(cov).requires_grad_(True)
        kw.update(colors_precomp=tc, cov3D_precomp=tv)
    else:
        kw.update(shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    color, radii, depth, alpha = GaussianRasterizer(st)(**kw)
    loss = sum((o * _dev(g)).sum() for o, g in ((color, gC), (depth, gD), (alpha, gA)) if g is not None)
    loss.backward()
    torch.cuda.synchronize()
    if outputs is not None:
        outputs.update(color=color.detach(), radii=radii, depth=depth.detach(), alpha=alpha.detach(), oracle=ro, oracle_radii=o_out[1],
                       colors_precomp=None if tc is None else tc.grad, cov3D_precomp=None if tv is None else tv.grad)

    # The fork's backward derives every T_j from T_final := 1 - alpha_out: at a nearly opaque pixel (alpha 0.9999) a
    # 1-ulp difference of the two forwards' alpha images (fp32 summation order) is a 1e-3 relative difference of T_final.
    # So the backward is checked in isolation at `tol` (the oracle replays with THIS forward's alpha image, exactly the
    # input the fork's backward gets) and end to end at the looser bar that conditioning allows.
    go_iso = ro.backward(gC, gD, gA, alpha_out=alpha.detach().cpu().numpy().reshape(1, H, W))
    if outputs is not None:
        outputs["oracle_grads"] = go_iso

    def close(name, ours, ref, floor=0.0, bar=tol):
        # `floor`: magnitude below which a gradient is analytically zero (e.g. the rotation of an isotropic Gaussian)
        if geom_tol is not None and name in ("means3D", "scales", "rotations", "cov3D_precomp"):
            bar = max(bar, geom_tol)      # covariance path of pathological needles: fp32 second moments (see the caller)
        err = _max_norm_error(ours.detach().cpu().numpy(), ref, floor)
        assert err < bar, "%s: max error / max |grad| = %.3e" % (name, err)

    for go, bar in ((go_iso, tol), (go_e2e, max(tol, tol_e2e))):
        close("means3D", t["means3D"].grad, go["means3D"], bar=bar)
        close("means2D", means2D.grad, go["means2D"], bar=bar)
        close("opacities", t["opacities"].grad, go["opacities"], bar=bar)
        if use_precomp:
            close("colors_precomp", tc.grad, go["colors_precomp"], bar=bar)
            close("cov3D_precomp", tv.grad, go["cov3D_precomp"], bar=bar)
        else:
            close("shs", t["shs"].grad, go["shs"], bar=bar)
            close("scales", t["scales"].grad, go["scales"], bar=bar)
            close("rotations", t["rotations"].grad, go["rotations"],
                  floor=float(np.abs(go["scales"] * sc["scales"]).max()), bar=bar)
    return t, means2D


def test_backward_parity_exact_lists(oracle, monkeypatch):
    monkeypatch.setenv("GIP_RASTER_EXACT_LISTS", "1")
    _check_backward(oracle, "stress", 2500, 96, 80, 12, 1)


@pytest.mark.parametrize("kind,P,H,W,seed,deg", [("stress", 1500, 64, 64, 11, 0), ("stress", 2500, 96, 80, 12, 1),
                                                 ("stress", 1200, 64, 96, 13, 3), ("ball", 10000, 256, 256, 42, 0)])
def test_backward_parity(oracle, kind, P, H, W, seed, deg):
    _check_backward(oracle, kind, P, H, W, seed, deg)


def test_backward_parity_precomputed_inputs(oracle):
    _check_backward(oracle, "stress", 1500, 72, 72, 21, 0, use_precomp=True)


def test_backward_is_bitwise_reproducible(oracle):
    a, m_a = _check_backward(oracle, "stress", 3000, 96, 96, 31, 1)
    b, m_b = _check_backward(oracle, "stress", 3000, 96, 96, 31, 1)
    for k in ("means3D", "opacities", "shs", "scales", "rotations"):
        assert torch.equal(a[k].grad, b[k].grad), k
    assert torch.equal(m_a.grad, m_b.grad)


@pytest.mark.parametrize("sh_path", ["scalar", "matrix cores"])
def test_multiview_equals_single_views(oracle, monkeypatch, sh_path):
    """One launch set of four views against four single-view calls.  With the scalar SH chain (GIP_RASTER_SH_SCALAR=1) the images
    are bit-identical; by default the launch set contracts its SH colours on the matrix cores (csrc/sh_mfma.hip) while a single
    view has nothing to batch and stays scalar: colours then differ by rounding (a few ulp), images by < 1e-5."""
    from gaussianip_amd import GaussianRasterizer, rasterize_views
    monkeypatch.setenv("GIP_RASTER_SH_SCALAR", "1" if sh_path == "scalar" else "0")
    same = torch.equal if sh_path == "scalar" else (lambda a, b: bool((a - b).abs().max() < 1e-5))
    P, H, W = 4000, 96, 128
    sc = scenes.make_scene("stress", P, seed=5, sh_degree=1)
    cams = scenes.train_cameras(4, 9, H, W)
    sts = [_settings(c, H, W, (0.0, 0.0, 0.0), 1) for c in cams]
    t = {k: _dev(v).requires_grad_(True) for k, v in sc.items()}
    m2 = torch.zeros(4, P, 3, device="cuda", requires_grad=True)
    color, radii, depth, alpha = rasterize_views(t["means3D"], m2, t["opacities"], sts, shs=t["shs"], scales=t["scales"],
                                                 rotations=t["rotations"])
    g = torch.Generator(device="cuda").manual_seed(3)
    gC = torch.randn(color.shape, device="cuda", generator=g)
    gD = torch.randn(depth.shape, device="cuda", generator=g)
    ((color * gC).sum() + (depth * gD).sum()).backward()
    batched = {k: v.grad.clone() for k, v in t.items()}
    m2g = m2.grad.clone()
    for v_ in t.values():
        v_.grad = None
    singles2d = []
    for i, s in enumerate(sts):
        m = torch.zeros(P, 3, device="cuda", requires_grad=True)
        c1, r1, d1, a1 = GaussianRasterizer(s)(means3D=t["means3D"], means2D=m, opacities=t["opacities"], shs=t["shs"],
                                               scales=t["scales"], rotations=t["rotations"])
        assert same(c1, color[i]) and torch.equal(d1, depth[i]) and torch.equal(a1, alpha[i])
        assert torch.equal(r1, radii[i])
        ((c1 * gC[i]).sum() + (d1 * gD[i]).sum()).backward()
        singles2d.append(m.grad)
    if sh_path == "scalar":
        assert torch.equal(torch.stack(singles2d), m2g)
    else:
        assert float((torch.stack(singles2d) - m2g).abs().max() / m2g.abs().max()) < 1e-5
    for k in t:
        ref = t[k].grad
        scale = ref.abs().max() + 1e-20
        assert ((batched[k] - ref).abs().max() / scale) < 1e-5, k


def test_errors_and_edge_cases(oracle):
    from gaussianip_amd import GaussianRasterizer
    H = W = 32
    cam = scenes.camera(0.0, 0.0, 2.0, 60.0, H, W)
    st = _settings(cam, H, W, (0.5, 0.25, 0.75), 0)
    sc = scenes.make_scene("ball", 64, seed=1)
    t = {k: _dev(v) for k, v in sc.items()}
    rast = GaussianRasterizer(st)
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        rast(means3D=t["means3D"], means2D=None, opacities=t["opacities"], scales=t["scales"], rotations=t["rotations"])
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        rast(means3D=t["means3D"], means2D=None, opacities=t["opacities"], shs=t["shs"], scales=t["scales"])
    # all Gaussians behind the camera -> pure background, radii 0
    behind = t["means3D"].clone()
    behind[:, 0] += 10.0
    color, radii, depth, alpha = rast(means3D=behind, means2D=None, opacities=t["opacities"], shs=t["shs"],
                                      scales=t["scales"], rotations=t["rotations"])
    assert int(radii.abs().sum()) == 0 and float(alpha.abs().max()) == 0.0
    assert torch.allclose(color[:, 0, 0], torch.tensor([0.5, 0.25, 0.75], device="cuda"))
    # empty input
    e = torch.zeros(0, 3, device="cuda")
    color, radii, depth, alpha = rast(means3D=e, means2D=None, opacities=torch.zeros(0, 1, device="cuda"),
                                      shs=torch.zeros(0, 1, 3, device="cuda"), scales=e, rotations=torch.zeros(0, 4, device="cuda"))
    assert radii.numel() == 0 and torch.allclose(color[:, 5, 5], torch.tensor([0.5, 0.25, 0.75], device="cuda"))
    vis = rast.markVisible(t["means3D"])
    assert vis.dtype == torch.bool and bool(vis.all())


def _adversarial_scene(seed, translucent):
    """Needle-thin and huge splats (up to ~150:1, 12x), opacities around the 1/255 threshold (where the alpha region
    degenerates) on 30 % of the Gaussians, a close camera (big rectangles on both sides of the 32-tile mask limit, clipped
    ones, centres off screen).  `translucent`: the rest nearly transparent, so the image stays far from opaque."""
    rng = np.random.default_rng(100 + seed)
    P, H, W = 6000, 160, 208
    sc = scenes.make_scene("stress", P, seed=seed, sh_degree=1)
    sc["scales"] = (sc["scales"] * np.exp(rng.uniform(-2.5, 2.5, (P, 3)))).astype(np.float32)
    op = rng.uniform(0.0, 1.0, (P, 1))
    near = rng.random((P, 1)) < 0.3
    op[near] = (1.0 / 255.0) * np.exp(rng.uniform(-0.2, 0.6, int(near.sum())))
    if translucent:
        op[~near] *= 0.004
    sc["opacities"] = op.astype(np.float32)
    return sc, scenes.camera(12.0, 40.0 + 30.0 * seed, 0.9 + 0.4 * seed, 65.0, H, W), P, H, W


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_culled_lists_change_no_output_on_adversarial_scenes(monkeypatch, seed):
    """The instance / block / quadrant culling bounds must be conservative for ANY Gaussian.  Default (culled) mode against
    exact_lists mode — which the tests above pin to the oracle bit for bit — on a translucent adversarial scene (no
    T_final := 1 - alpha_out conditioning, so the two modes must agree to summation-order rounding): same radii, same
    images, same gradients."""
    from gaussianip_amd import rasterizer as R
    sc, cam, P, H, W = _adversarial_scene(seed, True)
    st = _settings(cam, H, W, (0.2, 0.1, 0.3), 1)
    g = torch.Generator(device="cuda").manual_seed(seed)
    gC = torch.randn(1, 3, H, W, device="cuda", generator=g)
    gD = torch.randn(1, 1, H, W, device="cuda", generator=g)
    gA = torch.randn(1, 1, H, W, device="cuda", generator=g)
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("GIP_RASTER_EXACT_LISTS", mode)
        t = {k: _dev(v).requires_grad_(True) for k, v in sc.items()}
        m2d = torch.zeros(1, P, 3, device="cuda", requires_grad=True)
        color, radii, depth, alpha = R.rasterize_views(t["means3D"], m2d, t["opacities"], [st], shs=t["shs"], scales=t["scales"],
                                                       rotations=t["rotations"])
        grads = torch.autograd.grad([color, depth, alpha], [t["means3D"], t["shs"], t["opacities"], t["scales"], t["rotations"], m2d],
                                    [gC, gD, gA])
        outs[mode] = (color.detach(), depth.detach(), alpha.detach(), radii, grads)
    torch.cuda.synchronize()
    ce, de, ae, re_, ge = outs["1"]
    cc, dc, ac, rc, gc = outs["0"]
    assert torch.equal(re_, rc) and float(ae.max()) < 0.97
    assert float((ce - cc).abs().max()) < 5e-6 and float((ae - ac).abs().max()) < 5e-6
    assert float((de - dc).abs().max()) < 5e-6 * max(1.0, float(de.abs().max()))
    # colour / opacity / screen-space gradients (first moments) agree to rounding; the covariance path of a 500-pixel needle
    # with an opacity at the threshold sums second moments (dx^2 ~ 1e5) with heavy cancellation and is then pushed through
    # a 1e5:1 conditioned covariance — there the two modes' different checkpoint positions (other segment boundaries in
    # the shorter lists) show as 1e-3-level fp32 noise, in both modes alike
    for name, a, b in zip(("means3D", "shs", "opacities", "scales", "rotations", "means2D"), ge, gc):
        bar = 2e-5 if name in ("shs", "opacities", "means2D") else 1e-2
        assert float((a - b).abs().max()) <= bar * float(a.abs().max()) + 1e-12, name


@pytest.mark.parametrize("seed,translucent", [(0, True), (1, False), (2, True), (3, False)])
def test_tile_lists_of_adversarial_scenes_lose_only_dead_entries(oracle, seed, translucent):
    """compare_tile_lists (every dropped entry fails the alpha test at all 256 pixels of its tile, brute force) and the
    image parity against the oracle on the adversarial Gaussians."""
    sc, cam, P, H, W = _adversarial_scene(seed, translucent)
    oracle.set_threads(8)
    try:
        _check_forward_scene(oracle, sc, cam, H, W, 1, bg=(0.2, 0.1, 0.3), nc_mismatch_frac=2e-3, min_keep=0.0)
    finally:
        oracle.set_threads(1)


@pytest.mark.parametrize("seed", [1, 3])
def test_backward_parity_on_opaque_adversarial_scenes(oracle, seed):
    """The same adversarial Gaussians, opaque (nearly every pixel ends at alpha 0.9999): default (culled) mode against the
    oracle with the backward isolated from the alpha image's rounding (see _check_backward), the end-to-end bar widened
    to what T_final := 1 - alpha_out allows when the WHOLE image is at the 0.9999 cap."""
    sc, cam, P, H, W = _adversarial_scene(seed, False)
    oracle.set_threads(8)
    try:
        # colour / opacity / screen-space gradients at the usual 2e-3; the covariance path of 500-pixel needles (second
        # moments with dx^2 ~ 1e5 summed in fp32 by the library, in double by the oracle, then a 1e5:1 conditioned
        # covariance) at 5e-2
        # (1e-2 instead of 2e-3 for the rest: a third of these Gaussians sit AT the alpha threshold, so libm expf and
        # v_exp_f32 decide the alpha >= 1/255 test differently at more pixels than in any realistic scene)
        _check_backward(oracle, "stress", P, H, W, seed, 1, scene=sc, cam=cam, tol=1e-2, tol_e2e=1e-1, geom_tol=5e-2)
    finally:
        oracle.set_threads(1)


def test_forward_only_render_is_bit_identical_and_keeps_nothing_for_a_backward(monkeypatch):
    """GipRasterConfig::forward_only (set for renders under torch.no_grad()): same images and radii bit for bit, long tile
    lists included (several 64-entry segments per tile = checkpoints skipped), and the C entry point refuses a backward on
    such a state."""
    import ctypes
    from gaussianip_amd import _lib, rasterize_views
    from gaussianip_amd import rasterizer as rz
    P, H, W = 20000, 128, 160
    sc = scenes.make_scene("stress", P, seed=11, sh_degree=1)
    cams = scenes.train_cameras(3, 4, H, W)
    sts = [_settings(c, H, W, (0.1, 0.2, 0.3), 1) for c in cams]
    t = {k: _dev(v) for k, v in sc.items()}

    def render(grad):
        tt = {k: v.clone().requires_grad_(grad) for k, v in t.items()}
        ctx = torch.enable_grad() if grad else torch.no_grad()
        with ctx:
            return rasterize_views(tt["means3D"], None, tt["opacities"], sts, shs=tt["shs"], scales=tt["scales"], rotations=tt["rotations"])
    seen = []
    orig = rz._run_forward
    monkeypatch.setattr(rz, "_run_forward", lambda plan, cap, fo=False: (seen.append(bool(fo)), orig(plan, cap, fo))[1])
    with_state = render(True)
    without = render(False)
    assert seen[0] is False and seen[-1] is True, seen
    for a, b in zip(with_state, without):
        assert torch.equal(a, b)
    monkeypatch.setenv("GIP_RASTER_FORWARD_ONLY", "0")
    again = render(False)
    assert seen[-1] is False and all(torch.equal(a, b) for a, b in zip(with_state, again))
    # the C-ABI refuses a backward on a state whose forward kept nothing
    monkeypatch.setattr(rz, "_run_forward", orig)
    monkeypatch.delenv("GIP_RASTER_FORWARD_ONLY")
    plan = rz._build_plan(t["means3D"], t["shs"], None, t["opacities"], t["scales"], t["rotations"], None, sts)
    color, radii, depth, alpha = rz._forward_with_policy(plan, False, forward_only=True)
    assert plan.cfg.forward_only == 1 and torch.equal(color, with_state[0])
    with pytest.raises(ValueError):
        rz._run_backward(plan, (color, depth, alpha), torch.ones_like(color), None, None)
