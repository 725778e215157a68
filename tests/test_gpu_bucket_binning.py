"""Bucket mode of the tile binning against the dense layout it replaces on the hot path.

In bucket mode tile t of a launch set keeps its keys at bucket_keys[t * S ..) (S = the stride the host policy derives from the
previous call's longest list), the preprocess kernel stores every key itself and no scatter launch runs.  Keys are unique, so
the sorted lists — and every buffer and output behind them — must equal the dense path's BIT FOR BIT: that is what these
tests assert, with both modes forced by GIP_RASTER_BUCKETS inside one process, on lists of 1, 63, 64, 65, 511, 512, 513 and
2100 entries (every size class of the tile sort and its thresholds) and Gaussians of 1, 8, 9 and more than 32 tiles (the
remembered slots, the first instance beyond them, the rectangles without a tile mask).  Then: a bucket exactly full and one
entry over (the overflow protocol), the oracle's bars on a small scene rendered in bucket mode, and degenerate inputs."""
import warnings

import numpy as np
import pytest
import torch

import bucket_scenes as bs
import scenes
from test_gpu_raster_parity import _check_backward, _check_forward_scene, _dev, _settings

pytestmark = pytest.mark.gpu
GRADS = ("means3D", "means2D", "opacities", "shs", "scales", "rotations")
AZIMUTHS = (0.0, 7.0, -5.0)
_dense_cache = {}


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


def _upstream(seed, V, H, W):
    rng = np.random.default_rng(seed)
    return tuple(_dev(rng.normal(size=(V, c, H, W)).astype(np.float32)) for c in (3, 1, 1))


def _render(sc, sts, H, W, plans, monkeypatch, mode):
    """Forward + backward of the launch set in the given key layout.  Returns every compared array as numpy."""
    from gaussianip_amd import rasterizer as R
    from gaussianip_amd import rasterize_views
    V, P = len(sts), sc["means3D"].shape[0]
    monkeypatch.setenv("GIP_RASTER_BUCKETS", "1" if mode == "bucket" else "0")
    t = {k: _dev(v).requires_grad_(True) for k, v in sc.items()}
    kw = dict(shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    key = R._bucket_key(R._hint_key(t["means3D"].device, P, V, H, W))
    if mode == "bucket" and key not in R._bucket_hint:             # the first call of a shape is dense and leaves the hint
        with torch.no_grad():
            rasterize_views(t["means3D"], None, t["opacities"], sts, **kw)
    hint = R._bucket_hint.get(key)
    m2 = torch.zeros(V, P, 3, device="cuda", requires_grad=True)
    color, radii, depth, alpha = rasterize_views(t["means3D"], m2, t["opacities"], sts, **kw)
    plan = plans[-1]
    assert plan.bucket_stride == (R.bucket_stride(hint) if mode == "bucket" else 0), (mode, hint, plan.bucket_stride)
    g = torch.autograd.grad([color, depth, alpha], [t["means3D"], m2, t["opacities"], t["shs"], t["scales"], t["rotations"]],
                            list(_upstream(23, V, H, W)))
    torch.cuda.synchronize()
    sv = R.state_views(plan)
    hdr = sv["header"].cpu().numpy()
    n = int(hdr[1])
    out = dict(color=color, depth=depth, alpha=alpha, radii=radii, keys=sv["keys"][:n], tile_start=sv["tile_start"],
               header=sv["header"][1:6], inst_offset=sv["inst_offset"], n_contrib=sv["n_contrib"], tiles=sv["records_u32"][:, :, 7])
    out.update({"grad_" + k: v for k, v in zip(GRADS, g)})
    out = {k: v.detach().cpu().numpy() for k, v in out.items()}
    if mode == "bucket":
        assert int(hdr[13]) == plan.bucket_stride                  # the forward records the stride in reserved[0]
        assert int(hdr[3]) <= plan.bucket_stride and R._bucket_hint[key] == max(hint, int(hdr[3]))      # the hint is only raised
    return out


def _assert_equal(a, b, what):
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), "%s: %s differs" % (what, k)
    for k in GRADS:
        assert np.isfinite(a["grad_" + k]).all() and float(np.abs(a["grad_" + k]).max()) > 0.0, k


CASES = {                      #  views  exact lists  antialiased
    "1 view": (1, False, False), "3 views": (3, False, False), "1 view / exact lists": (1, True, False),
    "3 views / exact lists": (3, True, False), "1 view / antialiased": (1, False, True)}


def _case(name, plans, monkeypatch, mode):
    V, exact, aa = CASES[name]
    monkeypatch.setenv("GIP_RASTER_EXACT_LISTS", "1" if exact else "0")
    sc = bs.list_scene()
    sts = [_settings(bs.camera(az), bs.H, bs.W, bs.BG, bs.SH_DEGREE)._replace(antialiasing=aa) for az in AZIMUTHS[:V]]
    if mode == "dense":
        if name not in _dense_cache:
            _dense_cache[name] = _render(sc, sts, bs.H, bs.W, plans, monkeypatch, "dense")
        return _dense_cache[name]
    return _render(sc, sts, bs.H, bs.W, plans, monkeypatch, "bucket")


@pytest.mark.parametrize("name", list(CASES))
def test_bucket_mode_equals_dense_bit_for_bit(plans, monkeypatch, name):
    """Colour, depth, alpha, radii, the six gradients, the compacted keys, tile_start, inst_offset, n_contrib and header
    words 1-5 of the two layouts are identical."""
    dense = _case(name, plans, monkeypatch, "dense")
    bucket = _case(name, plans, monkeypatch, "bucket")
    _assert_equal(bucket, dense, name)
    ts = dense["tile_start"].astype(np.int64)
    lengths = set((ts[1:] - ts[:-1]).tolist())
    tiles = set(dense["tiles"][0].tolist())
    print(name, "list lengths", sorted(lengths)[-12:], "tiles per Gaussian", sorted(tiles))
    assert int(dense["header"][1]) == 0                                            # no overflow
    # the scene reaches what it is there for (view 0 is the camera the lists were built for)
    assert set(bs.LENGTHS) <= lengths, sorted(lengths)
    assert {1, 8, 9} <= tiles and max(tiles) > 32, sorted(tiles)


def test_bucket_mode_is_bitwise_reproducible(plans, monkeypatch):
    a = _case("3 views", plans, monkeypatch, "bucket")
    b = _case("3 views", plans, monkeypatch, "bucket")
    _assert_equal(a, b, "bucket mode twice")


def _one_tile_scene(n):
    """64 x 64 pixels: n one-tile splats in tile (1, 1), three in tile (2, 2)."""
    rng = np.random.default_rng(n)
    cam = scenes.camera(0.0, 0.0, 2.0, 40.0, 64, 64)
    fx = 64 / (2.0 * cam["tanfovx"])
    z = 2.0 + rng.permutation(n + 3) * 1e-3
    px = np.r_[np.full(n, 23.5), np.full(3, 39.5)]

    def world(px, py, z):
        nx, ny = (2.0 * px + 1.0) / 64 - 1.0, (2.0 * py + 1.0) / 64 - 1.0
        pv = np.stack([nx * z * cam["tanfovx"], ny * z * cam["tanfovy"], z, np.ones_like(z)], -1)
        return (pv @ np.linalg.inv(cam["viewmatrix"].astype(np.float64)))[..., :3]
    P = n + 3
    rot = np.zeros((P, 4), np.float32)
    rot[:, 0] = 1
    shs = np.zeros((P, 1, 3), np.float32)
    shs[:, 0, :] = rng.uniform(-1, 1, (P, 3))
    sc = dict(means3D=world(px, px, z).astype(np.float32), scales=np.repeat((z / fx)[:, None], 3, 1).astype(np.float32), rotations=rot,
              opacities=rng.uniform(0.01, 0.03, (P, 1)).astype(np.float32), shs=shs)
    return sc, cam


@pytest.mark.parametrize("n,over", [(96, False), (97, True)])
def test_a_full_bucket_and_one_entry_over(plans, monkeypatch, n, over):
    """Stride 96 (a longest-list hint of 16).  A list of exactly 96 entries fills its bucket: no overflow, equal to dense.  97:
    the header's overflow flag, a zero-gradient step, the bucket's own warning, the hint raised — and the next call, in
    bucket mode again, equals dense."""
    from gaussianip_amd import rasterizer as R
    sc, cam = _one_tile_scene(n)
    sts = [_settings(cam, 64, 64, bs.BG, 0)]
    dense = _render(sc, sts, 64, 64, plans, monkeypatch, "dense")
    ts = dense["tile_start"].astype(np.int64)
    assert int((ts[1:] - ts[:-1]).max()) == n and int(dense["header"][2]) == n
    key = R._bucket_key(R._hint_key(torch.device("cuda", torch.cuda.current_device()), n + 3, 1, 64, 64))
    R._bucket_hint[key] = 16
    assert R.bucket_stride(16) == 96
    events = R.overflow_events
    if not over:
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            full = _render_with_stride(sc, sts, plans, monkeypatch, 96)
        _assert_equal(full, dense, "full bucket")
        assert R.overflow_events == events
        return
    with pytest.warns(RuntimeWarning, match="outgrew its bucket of 96"):
        cut = _render_with_stride(sc, sts, plans, monkeypatch, 96)
    assert int(cut["header"][1]) == 1 and int(cut["header"][2]) == 97 and int(cut["header"][0]) == 100
    for k in GRADS:
        assert np.isfinite(cut["grad_" + k]).all() and float(np.abs(cut["grad_" + k]).max()) == 0.0, k
    assert R.overflow_events == events + 1 and R._bucket_hint[key] == 97
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        again = _render_with_stride(sc, sts, plans, monkeypatch, R.bucket_stride(97))
    _assert_equal(again, dense, "the call after the overflow")


def _render_with_stride(sc, sts, plans, monkeypatch, stride):
    """Bucket mode with the stride the present hint gives; the overflowed call is allowed its zero gradients."""
    from gaussianip_amd import rasterizer as R
    from gaussianip_amd import rasterize_views
    monkeypatch.setenv("GIP_RASTER_BUCKETS", "1")
    P = sc["means3D"].shape[0]
    t = {k: _dev(v).requires_grad_(True) for k, v in sc.items()}
    m2 = torch.zeros(1, P, 3, device="cuda", requires_grad=True)
    color, radii, depth, alpha = rasterize_views(t["means3D"], m2, t["opacities"], sts, shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    plan = plans[-1]
    assert plan.bucket_stride == stride
    g = torch.autograd.grad([color, depth, alpha], [t["means3D"], m2, t["opacities"], t["shs"], t["scales"], t["rotations"]],
                            list(_upstream(23, 1, 64, 64)))
    torch.cuda.synchronize()
    sv = R.state_views(plan)
    n = min(int(sv["header"][1]), sv["keys"].numel())
    out = dict(color=color, depth=depth, alpha=alpha, radii=radii, keys=sv["keys"][:n], tile_start=sv["tile_start"],
               header=sv["header"][1:6], inst_offset=sv["inst_offset"], n_contrib=sv["n_contrib"], tiles=sv["records_u32"][:, :, 7])
    out.update({"grad_" + k: v for k, v in zip(GRADS, g)})
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def test_oracle_parity_in_bucket_mode(oracle, plans, monkeypatch):
    """The forward's integer buffers and images and the backward's gradients against the CPU oracle, with the bars of
    test_gpu_raster_parity.py, on calls that the policy ran in bucket mode."""
    from gaussianip_amd import rasterizer as R
    monkeypatch.setenv("GIP_RASTER_BUCKETS", "1")
    H, W, deg = 96, 80, 1
    sc = scenes.make_scene("stress", 2500, seed=12, sh_degree=deg)
    cam = scenes.camera(8.0, 60.0, 1.7, 60.0, H, W)
    with torch.no_grad():                                                          # the shape's first call: dense, leaves the hint
        R.forward_with_state(_dev(sc["means3D"]), _dev(sc["opacities"]), [_settings(cam, H, W, (0.0, 0.0, 0.0), deg)], shs=_dev(sc["shs"]),
                             scales=_dev(sc["scales"]), rotations=_dev(sc["rotations"]))
    first = len(plans)
    _check_forward_scene(oracle, sc, cam, H, W, deg)
    _check_backward(oracle, "stress", 2500, H, W, 12, deg, scene=sc, cam=cam)
    assert len(plans) >= first + 2 and all(p.bucket_stride > 0 for p in plans[first:]), [p.bucket_stride for p in plans]


def test_degenerate_inputs_in_bucket_mode(plans, monkeypatch):
    """No Gaussians at all, and a launch set with a view that sees nothing."""
    from gaussianip_amd import rasterizer as R
    from gaussianip_amd import rasterize_views
    monkeypatch.setenv("GIP_RASTER_BUCKETS", "1")
    H = W = 64
    cams = [scenes.camera(0.0, 0.0, 2.0, 40.0, H, W), scenes.camera(0.0, 180.0, 2.0, 40.0, H, W)]
    sts = [_settings(c, H, W, bs.BG, 0) for c in cams]
    bg = np.asarray(bs.BG, np.float32)
    empty = dict(means3D=torch.zeros(0, 3), opacities=torch.zeros(0, 1), shs=torch.zeros(0, 1, 3), scales=torch.zeros(0, 3),
                 rotations=torch.zeros(0, 4))
    empty = {k: v.cuda() for k, v in empty.items()}
    for i in range(2):                                                             # dense, then bucket mode
        with torch.no_grad():
            color, radii, depth, alpha = rasterize_views(empty["means3D"], None, empty["opacities"], sts[:1], shs=empty["shs"],
                                                         scales=empty["scales"], rotations=empty["rotations"])
        torch.cuda.synchronize()
        assert (plans[-1].bucket_stride > 0) == (i == 1)
        assert radii.shape == (1, 0) and float(alpha.abs().max()) == 0.0
        assert np.array_equal(color[0].cpu().numpy(), np.broadcast_to(bg[:, None, None], (3, H, W)))
    # 200 splats behind the second camera (in front of the first, three times as far)
    rng = np.random.default_rng(9)
    sc = scenes.make_scene("stress", 200, seed=9, sh_degree=0)
    sc["means3D"] = (sc["means3D"] * 0.3 + 2.0 * cams[1]["campos"][None, :]).astype(np.float32)
    res = {}
    for mode in ("dense", "bucket"):
        res[mode] = _render(sc, sts, H, W, plans, monkeypatch, mode)
    _assert_equal(res["bucket"], res["dense"], "a view with nothing visible")
    assert int(res["dense"]["radii"][1].max()) == 0 and int(res["dense"]["radii"][0].max()) > 0
    assert np.array_equal(res["bucket"]["color"][1], np.broadcast_to(bg[:, None, None], (3, H, W)))
    del rng, R
