"""The matrix-core SH path (csrc/sh_mfma.hip) on launch sets the other tests do not reach, against the CPU oracle — and the scalar
chain (GIP_RASTER_SH_SCALAR=1) beside it on every case:

  * Gaussians culled in SOME views of a set and visible in others: a mean at a camera's own position (the view direction is
    0 / 0 there), behind one camera, outside one camera's frustum; and Gaussians behind every camera, which get exact zeros;
  * launch sets of 3 / 5 / 8 / 12 / 16 views (ragged last groups of the four-view MFMA blocks, GIP_MAX_VIEWS) and a 17-view call;
  * ragged Gaussian counts (1, 63, 65, 64 m + 1: the clamped index and the tail workgroup of the 64-Gaussian kernels);
  * a capacity overflow of a four-view degree-3 set: the matrix-core backward returns early and every gradient is zero.

Reference per view: the oracle's images and radii; parameter gradients are the oracle's per-view gradients summed over the views in
float64.  Bars: radii bit-exact, images those of test_gpu_raster_parity.py, gradients those of test_gpu_headline_parity.py
(`_compare`); the two SH paths agree at test_gpu_sh_mfma.py's bars."""
import ctypes

import numpy as np
import pytest
import torch

import scenes
import test_gpu_headline_parity as hp
from test_gpu_raster_parity import _assert_images, _dev, _oracle_forward, _settings
from test_gpu_sh_mfma import _run

pytestmark = pytest.mark.gpu

H, W = 128, 160
BG = (0.1, 0.2, 0.3)
PATHS = ["matrix cores", "scalar"]
GRADS = ("means2D", "g_means3D", "g_opacities", "g_shs", "g_scales", "g_rotations")


def _upstream(V, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(V, 3, H, W)).astype(np.float32), rng.normal(size=(V, 1, H, W)).astype(np.float32)


def _sh_path(monkeypatch, sh_path):
    monkeypatch.setenv("GIP_RASTER_SH_SCALAR", "1" if sh_path == "scalar" else "0")


def _against_oracle(oracle, sc, cams, deg, gC, gD, tag, want_state=False):
    """One launch set through rasterize_views (test_gpu_sh_mfma._run) against the oracle, view by view.  Returns (our outputs,
    oracle radii [V, P], oracle gradients summed over the views)."""
    V, P = len(cams), sc["means3D"].shape[0]
    sts = [_settings(c, H, W, BG, deg) for c in cams]
    got = _run(sc, sts, _dev(gC), _dev(gD), want_state=want_state)
    torch.cuda.synchronize()
    nonfinite = {}
    for k in ("color", "depth", "alpha") + GRADS:
        bad = ~torch.isfinite(got[k])
        if bool(bad.any()):                 # Gaussian rows (gradients) or pixels (images) holding NaN / Inf
            rows = bad.reshape(bad.shape[0], -1).any(1) if k != "means2D" else bad.any(0).any(1)
            nonfinite[k] = rows.nonzero().flatten().tolist()[:12]
    assert not nonfinite, "%s: non-finite entries (rows / views) %s" % (tag, nonfinite)
    alpha_np = got["alpha"].cpu().numpy()
    gA = np.zeros((1, H, W), np.float32)
    oracle.set_threads(oracle.max_threads())
    try:
        imgs, grads, ros = [], [], []
        for v, cam in enumerate(cams):
            ro, out = _oracle_forward(oracle, sc, cam, H, W, BG, deg)
            imgs.append(out)
            ros.append(ro)
            grads.append(ro.backward(gC[v], gD[v], gA, alpha_out=alpha_np[v]))
        kd = [ro.knife_edge_gaussians(sharing=True) for ro in ros]
    finally:
        oracle.set_threads(1)
    knife, behind = [k[0] for k in kd], [k[2] for k in kd]
    knife_any, behind_any = np.logical_or.reduce(knife), np.logical_or.reduce(behind)
    for v in range(V):
        o_color, o_radii, o_depth, o_alpha = imgs[v]
        assert np.array_equal(got["radii"][v].cpu().numpy(), o_radii), "%s: radii of view %d" % (tag, v)
        _assert_images(ros[v], got["color"][v], got["depth"][v], got["alpha"][v], o_color, o_depth, o_alpha)
        hp._compare(tag, "means2D[%d]" % v, got["means2D"][v], grads[v]["means2D"], skip_rows=knife[v], loose_rows=behind[v])
    tot = {k: sum(g[k].astype(np.float64) for g in grads) for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    M = sc["shs"].shape[1]
    for k in ("means3D", "opacities", "shs", "scales"):
        hp._compare(tag, k, got["g_" + k], tot[k], skip_rows=knife_any, loose_rows=behind_any,
                    max_loose=hp.MAX_LOOSE_ENTRIES * (M if k == "shs" else 1))
    hp._compare(tag, "rotations", got["g_rotations"], tot["rotations"], floor=float(np.abs(tot["scales"] * sc["scales"]).max()),
                skip_rows=knife_any, loose_rows=behind_any)
    return got, np.stack([im[1] for im in imgs]), tot


def _two_paths_agree(got, ref, tag):
    """test_gpu_sh_mfma.py's bars between the matrix-core path (`got`) and the scalar chain (`ref`)."""
    assert torch.equal(got["radii"], ref["radii"]), tag
    for k in ("color", "depth", "alpha"):
        assert float((got[k] - ref[k]).abs().max()) < 1e-5, (tag, k)
    for k in GRADS:
        top = float(ref[k].abs().max()) + 1e-30
        err = float((got[k] - ref[k]).abs().max()) / top
        assert err < 1e-5, (tag, k, err)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. Gaussians culled in some views of a launch set
# ---------------------------------------------------------------------------------------------------------------------------

def _arc_cameras(V, seed):
    """V cameras on a 150-degree arc of azimuths around the scene: every camera position lies in one half-space, so a point far
    out beyond them is behind all of them; the two end cameras see each other's positions."""
    rng = np.random.default_rng(seed)
    az0 = rng.uniform(-180, 180)
    return [scenes.camera(rng.uniform(-20, 20), az0 + 150.0 * i / (V - 1), rng.uniform(1.3, 1.7), rng.uniform(55, 70), H, W)
            for i in range(V)]


def _view_space(cams, p):
    """[V, N] view-space depth and [V, N] x / y NDC of the points p [N, 3] (float64 restatement of the preprocess transform)."""
    ph = np.concatenate([p.astype(np.float64), np.ones((len(p), 1))], 1)
    z = np.stack([ph @ c["viewmatrix"].astype(np.float64)[:, 2] for c in cams])
    hh = np.stack([ph @ c["projmatrix"].astype(np.float64) for c in cams])
    with np.errstate(divide="ignore", invalid="ignore"):
        return z, hh[..., 0] / hh[..., 3], hh[..., 1] / hh[..., 3]


def _plant(sc, cams, seed):
    """Overwrites rows of the scene with small (scale 0.01) Gaussians of four kinds and returns [(row, kind, k)]:
      (i)   mean = camera k's campos, bit for bit (the direction of view k is 0 / 0);
      (ii)  behind camera k only;
      (iii) in front of every camera, but far outside camera k's frustum;
      (iv)  behind every camera (k = -1).
    Kinds (i) - (iii) are planted only where another view has the point well inside its image (|NDC| < 0.7, depth > 0.5)."""
    V, P = len(cams), sc["means3D"].shape[0]
    rng = np.random.default_rng(seed)
    near = rng.uniform(-3.5, 3.5, (200000, 3))
    far = rng.normal(size=(50000, 3))
    far *= rng.uniform(4.0, 12.0, (50000, 1)) / np.linalg.norm(far, axis=1, keepdims=True)
    zn, xn, yn = _view_space(cams, near)
    seen = (zn > 0.5) & (np.abs(xn) < 0.7) & (np.abs(yn) < 0.7)
    front = zn > 0.5
    off = front & ((np.abs(xn) > 2.0) | (np.abs(yn) > 2.0))
    zc, xc, yc = _view_space(cams, np.stack([c["campos"] for c in cams]))
    seen_c = (zc > 0.5) & (np.abs(xc) < 0.7) & (np.abs(yc) < 0.7)
    plants = []
    for k in range(V):
        others = [j for j in range(V) if j != k]
        if seen_c[others, k].any():
            plants += [(cams[k]["campos"], "i", k)] * 2
        rest_seen = seen[others].any(0)
        for kind, ok in (("ii", (zn[k] < -0.3) & rest_seen), ("iii", off[k] & rest_seen)):
            # prefer points in front of every other camera (culled in view k only); else culled in k and some others
            pick = np.concatenate([np.flatnonzero(ok & front[others].all(0)), np.flatnonzero(ok & ~front[others].all(0))])
            plants += [(near[i], kind, k) for i in pick[:2]]
    zf = _view_space(cams, far)[0]
    plants += [(far[i], "iv", -1) for i in np.flatnonzero((zf < -0.5).all(0))[:4]]
    rows = rng.choice(P, len(plants), replace=False)           # scattered over the 64-Gaussian workgroups and their lanes
    out = []
    for r, (p, kind, k) in zip(rows, plants):
        sc["means3D"][r] = p
        sc["scales"][r] = 0.01
        sc["opacities"][r] = 0.7
        out.append((int(r), kind, k))
    return out


@pytest.mark.parametrize("sh_path", PATHS)
@pytest.mark.parametrize("V,deg", [(4, 1), (4, 2), (4, 3), (6, 1), (6, 2), (6, 3)])
def test_gaussians_culled_in_some_views_against_the_oracle(oracle, monkeypatch, sh_path, V, deg):
    _sh_path(monkeypatch, sh_path)
    P = 3000
    sc = scenes.make_scene("stress", P, seed=60 + 10 * V + deg, sh_degree=deg)
    cams = _arc_cameras(V, 7 + V)
    plants = _plant(sc, cams, seed=V + deg)
    kinds = {kd: [(r, k) for r, kind, k in plants if kind == kd] for kd in ("i", "ii", "iii", "iv")}
    assert len(kinds["i"]) >= 4 and len({k for _, k in kinds["i"]}) >= 2, kinds["i"]
    assert len({k for _, k in kinds["ii"]}) == V and len({k for _, k in kinds["iii"]}) == V and len(kinds["iv"]) == 4
    gC, gD = _upstream(V, 100 + V + deg)
    tag = "culled %d views / sh_degree %d (%s SH)" % (V, deg, sh_path)
    got, o_radii, tot = _against_oracle(oracle, sc, cams, deg, gC, gD, tag, want_state=True)
    radii = got["radii"].cpu().numpy()
    if sh_path == "matrix cores":        # the forward's colour buffer of every (view, Gaussian), culled pairs included, is finite
        from gaussianip_amd import _lib
        plan = got["plan"]
        L = _lib.GipRasterStateLayout()
        assert _lib.raster_lib().gip_raster_state_layout(ctypes.byref(plan.cfg), ctypes.byref(L)) == 0 and plan.cfg.sh_scalar == 0
        sh_colors = plan.state[L.sh_colors:L.sh_colors + V * P * 16].view(torch.float32).reshape(V, P, 4)
        assert bool(torch.isfinite(sh_colors).all()), [(kind, k, r) for r, kind, k in plants
                                                       if not bool(torch.isfinite(sh_colors[:, r]).all())]
    for r, kind, k in plants:
        if kind == "iv":
            assert not radii[:, r].any() and not o_radii[:, r].any(), (kind, r)
            for g in GRADS:
                t = got[g][:, r] if g == "means2D" else got[g][r]
                assert float(t.abs().max()) == 0.0, (tag, "row %d behind every camera: %s is not exactly zero" % (r, g))
            for g in ("means3D", "opacities", "shs", "scales", "rotations"):
                assert float(np.abs(tot[g][r]).max()) == 0.0, (g, r)
        else:                                   # not vacuous: culled in view k, drawn in another view
            assert radii[k, r] == 0 and (np.delete(radii[:, r], k) > 0).any(), (kind, k, r, radii[:, r])


@pytest.mark.parametrize("V,deg", [(4, 1), (4, 3), (6, 2), (6, 3)])
def test_culled_views_two_sh_paths_agree(monkeypatch, V, deg):
    P = 3000
    sc = scenes.make_scene("stress", P, seed=60 + 10 * V + deg, sh_degree=deg)
    cams = _arc_cameras(V, 7 + V)
    _plant(sc, cams, seed=V + deg)
    sts = [_settings(c, H, W, BG, deg) for c in cams]
    gC, gD = (_dev(a) for a in _upstream(V, 100 + V + deg))
    _sh_path(monkeypatch, "scalar")
    ref = _run(sc, sts, gC, gD)
    _sh_path(monkeypatch, "matrix cores")
    got = _run(sc, sts, gC, gD)
    _two_paths_agree(got, ref, "culled %d views / sh_degree %d" % (V, deg))


# ---------------------------------------------------------------------------------------------------------------------------
# 2. launch sets of more than 6 views
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh_path", PATHS)
@pytest.mark.parametrize("V,deg,P", [(3, 1, 20000), (5, 2, 16000), (8, 3, 12000), (12, 1, 12000), (16, 3, 10000)])
def test_view_counts_against_the_oracle(oracle, monkeypatch, sh_path, V, deg, P):
    _sh_path(monkeypatch, sh_path)
    sc = scenes.make_scene("stress", P, seed=70 + V, sh_degree=deg)
    cams = scenes.train_cameras(V, 30 + V, H, W)
    gC, gD = _upstream(V, 200 + V)
    got, _, _ = _against_oracle(oracle, sc, cams, deg, gC, gD, "%d views / sh_degree %d (%s SH)" % (V, deg, sh_path))
    assert bool((got["radii"] > 0).any(1).all())
    assert float(got["g_shs"][:, (deg + 1) ** 2 - 1].abs().max()) > 0


def test_seventeen_views_are_refused():
    from gaussianip_amd import rasterize_views
    P, deg = 500, 1
    sc = scenes.make_scene("stress", P, seed=3, sh_degree=deg)
    sts = [_settings(c, H, W, BG, deg) for c in scenes.train_cameras(17, 4, H, W)]
    t = {k: _dev(v) for k, v in sc.items()}
    with pytest.raises(ValueError, match="at most 16 views"):
        rasterize_views(t["means3D"], None, t["opacities"], sts, shs=t["shs"], scales=t["scales"], rotations=t["rotations"])


# ---------------------------------------------------------------------------------------------------------------------------
# 3. ragged Gaussian counts
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [1, 63, 65, 64 * 37 + 1])
def test_ragged_gaussian_counts(oracle, monkeypatch, P):
    V, deg = 4, 3
    full = scenes.make_scene("stress", 4096, seed=80, sh_degree=deg)
    sc = {k: np.ascontiguousarray(v[:P]) for k, v in full.items()}
    cams = scenes.train_cameras(V, 81, H, W)
    gC, gD = _upstream(V, 300 + P)
    out = {}
    for sh_path in PATHS:
        _sh_path(monkeypatch, sh_path)
        out[sh_path], _, _ = _against_oracle(oracle, sc, cams, deg, gC, gD, "P = %d (%s SH)" % (P, sh_path), want_state=True)
    got, ref = out["matrix cores"], out["scalar"]
    assert got["plan"].cfg.sh_scalar == 0 and ref["plan"].cfg.sh_scalar == 1
    assert bool((ref["radii"] > 0).any())
    # integer buffers identical between the two paths: radii, records' integer words, header, ranges, keys
    assert torch.equal(got["radii"], ref["radii"])
    ru, rr = got["views"]["records_u32"].cpu().numpy(), ref["views"]["records_u32"].cpu().numpy()
    for w in (7, 11, 12, 13, 15):
        assert np.array_equal(ru[..., w], rr[..., w]), "record word %d" % w
    n = int(ref["views"]["header"][1])
    assert int(got["views"]["header"][1]) == n and n > 0
    assert torch.equal(got["views"]["tile_start"], ref["views"]["tile_start"])
    assert torch.equal(got["views"]["keys"][:n], ref["views"]["keys"][:n])


# ---------------------------------------------------------------------------------------------------------------------------
# 4. capacity overflow of a matrix-core launch set
# ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh_path", PATHS)
@pytest.mark.parametrize("deg", [3, 1])
def test_capacity_overflow_of_a_four_view_degree3_set(monkeypatch, sh_path, deg):
    """Four views, coefficients stored for degree 3; the active degree 3 or 1 (then rows 4..15 of dL/dshs are inactive)."""
    from gaussianip_amd import rasterize_views
    from gaussianip_amd import rasterizer as R
    _sh_path(monkeypatch, sh_path)
    V, P = 4, 20000
    sc = scenes.make_scene("stress", P, seed=9, sh_degree=3)
    sts = [_settings(c, H, W, BG, deg) for c in scenes.train_cameras(V, 10, H, W)]
    t = {k: _dev(v).requires_grad_(True) for k, v in sc.items()}

    def render():
        return rasterize_views(t["means3D"], None, t["opacities"], sts, shs=t["shs"], scales=t["scales"], rotations=t["rotations"])[0]

    color_ref = render().detach().clone()
    key = R._hint_key(t["means3D"].device, P, V, H, W)
    true_r = R._capacity_hint[key]
    old_min, old_margin = R._MIN_CAPACITY, R._CAPACITY_MARGIN
    try:
        R._MIN_CAPACITY, R._CAPACITY_MARGIN = 1024, 0
        R._capacity_hint[key] = 100
        events = R.overflow_events
        color = render()
        with pytest.warns(RuntimeWarning, match="exceeded the capacity hint"):
            color.sum().backward()
        assert R.overflow_events == events + 1 and R._capacity_hint[key] == true_r
        for k, v in t.items():
            assert v.grad is not None and bool(torch.isfinite(v.grad).all()) and float(v.grad.abs().max()) == 0.0, k
            v.grad = None
        # the next call recovers: images bit for bit, live gradients in every coefficient row of the active degree
        c2 = render()
        c2.sum().backward()
        assert torch.equal(c2.detach(), color_ref)
        N = (deg + 1) ** 2
        assert float(t["shs"].grad[:, N - 1].abs().max()) > 0
        if N < 16:
            assert float(t["shs"].grad[:, N:].abs().max()) == 0.0
        assert float(t["means3D"].grad.abs().max()) > 0
    finally:
        R._MIN_CAPACITY, R._CAPACITY_MARGIN = old_min, old_margin
