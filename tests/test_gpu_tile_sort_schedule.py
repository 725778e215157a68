"""The tile sort's schedule (static first round of all three size classes, phase B's keys requested up front) must not change a
single key: keys are unique, so every tile's sorted list is one fixed permutation.

Scenes of stacked one-tile splats put lists of prescribed lengths into the tiles of a 64 x 64 and a 128 x 128 image: every
class and network edge of the sort (0, 1, 2, 64 | 65, 128 | 129, 256 | 257, 511 | 512, 513, 1023, 1024, 2047 | 2048, 2049 and
one list beyond the 16384-key chunk), every tenth splat at the depth of its neighbour so that the Gaussian index decides.  One
view and three views (one of the three looks away: every tile empty), both key layouts (GIP_RASTER_BUCKETS 0 / 1, the bucket
call behind the dense call that leaves the hint) and both list modes.  Two populations run the rounds behind the static one:
more class-A tiles than workgroups (the A cursor) and more than four class-M tiles per workgroup (the M cursor).

Asserted on keys / tile_start / header / seg_tile read through rasterizer.state_views: every list strictly ascending (equal depths
by index); in exact-lists mode the list of every tile equals the oracle's as a multiset; the two layouts agree bit for bit; seg_tile
names the tile of every segment; colour, depth, alpha and the six gradients are bitwise equal between two consecutive calls."""
import numpy as np
import pytest
import torch

import scenes
from test_gpu_raster_parity import _dev, _oracle_forward, _settings

pytestmark = pytest.mark.gpu
GRADS = ("means3D", "means2D", "opacities", "shs", "scales", "rotations")
BG = (0.3, 0.1, 0.2)
LONG_CHUNK = 16384
LENGTHS_128 = (0, 1, 2, 64, 65, 128, 129, 256, 257, 511, 512, 513, 1023, 1024, 2047, 2048, 2049, LONG_CHUNK + 1)
LENGTHS_64 = LENGTHS_128[:16]                                  # 4 x 4 tiles: up to 2048
SEGMENT = 64                                                   # GIP_SEGMENT


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


def _camera(size, azimuth=0.0):
    return scenes.camera(0.0, azimuth, 2.0, 40.0, size, size)


def _turned_away(cam):
    """The same camera turned half round about its own vertical axis: the scene lies behind it, every tile stays empty."""
    view = cam["viewmatrix"].astype(np.float64)
    proj = np.linalg.inv(view) @ cam["projmatrix"].astype(np.float64)
    view[:, 0] *= -1.0
    view[:, 2] *= -1.0
    return dict(cam, viewmatrix=view.astype(np.float32), projmatrix=(view @ proj).astype(np.float32))


def _world(cam, size, px, py, z):
    """World position of the point at view depth z that projects to pixel (px, py)."""
    nx, ny = (2.0 * px + 1.0) / size - 1.0, (2.0 * py + 1.0) / size - 1.0
    pv = np.stack([nx * z * cam["tanfovx"], ny * z * cam["tanfovy"], z, np.ones_like(z)], -1)
    return (pv @ np.linalg.inv(cam["viewmatrix"].astype(np.float64)))[..., :3]


def _pack(pos, scale, opac, rng):
    P = len(pos)
    rot = np.zeros((P, 4), np.float32)
    rot[:, 0] = 1
    shs = ((rng.uniform(0, 1, (P, 1, 3)) - 0.5) / 0.28209479177387814).astype(np.float32)
    return dict(means3D=pos.astype(np.float32), scales=scale.astype(np.float32), rotations=rot,
                opacities=opac.astype(np.float32)[:, None], shs=shs)


def _list_scene(size, lengths):
    """Tile i (row-major) of the camera at azimuth 0 holds exactly lengths[i] splats of radius 4 pixels around its centre."""
    rng = np.random.default_rng(size)
    cam = _camera(size)
    fx = size / (2.0 * cam["tanfovx"])
    tiles_x = size // 16
    pos, scale, opac = [], [], []
    for i, n in enumerate(lengths):
        if n == 0:
            continue
        z = 2.0 + rng.permutation(n) * (2e-4 if n < 4096 else 2e-5)
        z[1::10] = z[0:-1:10][:len(z[1::10])]                     # ties on depth: the index decides
        px = 16.0 * (i % tiles_x) + 7.5 + rng.uniform(-1.0, 1.0, n)
        py = 16.0 * (i // tiles_x) + 7.5 + rng.uniform(-1.0, 1.0, n)
        pos.append(_world(cam, size, px, py, z))
        scale.append(np.repeat((1.0 * z / fx)[:, None], 3, 1))    # sigma of one pixel: radius ceil(3 sqrt(1.3)) = 4
        opac.append(rng.uniform(0.006, 0.02, n))
    return _pack(np.concatenate(pos), np.concatenate(scale), np.concatenate(opac), rng)


def _filling_scene(size, n):
    """n Gaussians with a sigma of three image widths around the image centre: every tile of every view lists all of them."""
    rng = np.random.default_rng(n)
    cam = _camera(size)
    fx = size / (2.0 * cam["tanfovx"])
    z = 2.0 + rng.permutation(n) * 1e-4
    z[1::10] = z[0:-1:10][:len(z[1::10])]
    c = size / 2.0
    pos = _world(cam, size, c + rng.uniform(-8.0, 8.0, n), c + rng.uniform(-8.0, 8.0, n), z)
    scale = np.repeat((3.0 * size * z / fx)[:, None], 3, 1)
    return _pack(pos, scale, rng.uniform(0.006, 0.02, n), rng)


def _upstream(V, size):
    rng = np.random.default_rng(23)
    return [_dev(rng.normal(size=(V, c, size, size)).astype(np.float32)) for c in (3, 1, 1)]


def _render(sc, sts, size, plans, monkeypatch, mode):
    """Forward + backward of the launch set in the given key layout; every compared array as numpy."""
    from gaussianip_amd import rasterizer as R
    from gaussianip_amd import rasterize_views
    V, P = len(sts), sc["means3D"].shape[0]
    monkeypatch.setenv("GIP_RASTER_BUCKETS", "1" if mode == "bucket" else "0")
    t = {k: _dev(v).requires_grad_(True) for k, v in sc.items()}
    kw = dict(shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    key = R._bucket_key(R._hint_key(t["means3D"].device, P, V, size, size))
    if mode == "bucket" and key not in R._bucket_hint:             # the first call of a shape is dense and leaves the hint
        with torch.no_grad():
            rasterize_views(t["means3D"], None, t["opacities"], sts, **kw)
    m2 = torch.zeros(V, P, 3, device="cuda", requires_grad=True)
    color, radii, depth, alpha = rasterize_views(t["means3D"], m2, t["opacities"], sts, **kw)
    plan = plans[-1]
    assert (plan.bucket_stride > 0) == (mode == "bucket"), (mode, plan.bucket_stride)
    g = torch.autograd.grad([color, depth, alpha], [t["means3D"], m2, t["opacities"], t["shs"], t["scales"], t["rotations"]],
                            _upstream(V, size))
    torch.cuda.synchronize()
    sv = R.state_views(plan)
    hdr = sv["header"].cpu().numpy()
    assert int(hdr[2]) == 0, "overflow"
    state = dict(keys=sv["keys"][:int(hdr[1])], tile_start=sv["tile_start"], header=sv["header"][1:11], seg_tile=sv["seg_tile"][:int(hdr[5])])
    out = dict(color=color, depth=depth, alpha=alpha)
    out.update({"grad_" + k: v for k, v in zip(GRADS, g)})
    return {k: v.detach().cpu().numpy() for k, v in state.items()}, {k: v.detach().cpu().numpy() for k, v in out.items()}


def _assert_same(a, b, what):
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), "%s: %s differs" % (what, k)


def _check_lists(state, VT):
    """Strictly ascending lists (so equal depths are ordered by index) and the segment -> tile map.  Returns the lengths."""
    ts = state["tile_start"].astype(np.int64)
    keys = state["keys"].view(np.uint64)
    assert len(ts) == VT + 1 and ts[-1] == len(keys) == int(state["header"][0])
    lengths = ts[1:] - ts[:-1]
    tile_of = np.repeat(np.arange(VT), lengths)
    inner = tile_of[1:] == tile_of[:-1]                           # neighbours inside one list
    assert (keys[1:][inner] > keys[:-1][inner]).all(), "a tile's list is not strictly ascending"
    nseg = (lengths + SEGMENT - 1) // SEGMENT
    assert int(state["header"][4]) == int(nseg.sum())
    assert np.array_equal(state["seg_tile"].astype(np.int64), np.repeat(np.arange(VT), nseg)), "seg_tile"
    return lengths, tile_of, keys


def _check_against_oracle(oracle, sc, cams, size, state):
    """Exact-lists mode: tile by tile, view by view, the list is the oracle's as a multiset of (depth bits, Gaussian index)."""
    T = (size // 16) ** 2
    lengths, tile_of, keys = _check_lists(state, len(cams) * T)
    ties = 0
    for v, cam in enumerate(cams):
        ro, _ = _oracle_forward(oracle, sc, cam, size, size, BG, 0)
        okeys, vals, ranges, _tt, _nc = ro.binning()
        o_tile = (okeys >> np.uint64(32)).astype(np.int64)
        o_key = ((okeys & np.uint64(0xffffffff)) << np.uint64(32)) | vals.astype(np.uint64)
        o = np.stack([o_tile, o_key.view(np.int64)], 1)[np.lexsort((o_key, o_tile))]
        mine = tile_of // T == v
        m_key = keys[mine]
        m = np.stack([tile_of[mine] - v * T, m_key.view(np.int64)], 1)
        m = m[np.lexsort((m_key, m[:, 0]))]
        assert o.shape == m.shape and np.array_equal(o, m), "view %d: the lists are not the oracle's" % v
        d = m_key >> np.uint64(32)
        ties += int(((d[1:] == d[:-1]) & (m[1:, 0] == m[:-1, 0])).sum())
    assert ties > 0, "no equal depths inside a list: the scene does not test the tie order"
    return lengths


def _run(oracle, sc, cams, size, exact, plans, monkeypatch):
    monkeypatch.setenv("GIP_RASTER_EXACT_LISTS", "1" if exact else "0")
    sts = [_settings(c, size, size, BG, 0) for c in cams]
    VT = len(cams) * (size // 16) ** 2
    dense_state, dense_out = _render(sc, sts, size, plans, monkeypatch, "dense")
    bucket_state, bucket_out = _render(sc, sts, size, plans, monkeypatch, "bucket")
    again_state, again_out = _render(sc, sts, size, plans, monkeypatch, "bucket")
    for name, st in (("dense", dense_state), ("bucket", bucket_state)):
        lengths = _check_against_oracle(oracle, sc, cams, size, st) if exact else _check_lists(st, VT)[0]
    _assert_same(bucket_state, dense_state, "bucket against dense")
    _assert_same(bucket_out, dense_out, "bucket against dense")
    _assert_same(again_state, bucket_state, "two consecutive calls")
    _assert_same(again_out, bucket_out, "two consecutive calls")
    for k in GRADS:
        assert np.isfinite(bucket_out["grad_" + k]).all()
    return lengths, bucket_state["header"]


@pytest.mark.parametrize("exact", [False, True], ids=["default lists", "exact lists"])
@pytest.mark.parametrize("views", [1, 3])
@pytest.mark.parametrize("size", [64, 128])
def test_every_class_and_network_edge(oracle, plans, monkeypatch, size, views, exact):
    wanted = LENGTHS_64 if size == 64 else LENGTHS_128
    sc = _list_scene(size, wanted)
    cams = [_camera(size), _turned_away(_camera(size)), _camera(size, 7.0)][:views]
    lengths, header = _run(oracle, sc, cams, size, exact, plans, monkeypatch)
    T = (size // 16) ** 2
    assert tuple(lengths[:len(wanted)]) == wanted, lengths[:len(wanted)]         # view 0 is the camera the lists were built for
    if views == 3:
        assert (lengths[T:2 * T] == 0).all() and lengths[2 * T:].sum() > 0          # the view that looks away; the turned one


def test_more_long_lists_than_workgroups(oracle, plans, monkeypatch):
    """Six 128 x 128 views of 2100 screen-filling Gaussians: 384 tiles of class A, more than one per workgroup, so the rounds
    behind the static one draw from the A cursor."""
    size, n = 128, 2100
    cams = [_camera(size, az) for az in (0.0, 2.0, -2.0, 4.0, -4.0, 6.0)]
    lengths, header = _run(oracle, _filling_scene(size, n), cams, size, True, plans, monkeypatch)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert (lengths == n).all() and int(header[7]) == len(lengths) > cus          # class_end[1]: every tile is class A


def test_more_than_four_medium_lists_per_workgroup(oracle, plans, monkeypatch):
    """Six 256 x 256 views of 600 screen-filling Gaussians: 1536 tiles of class M, more than four per workgroup, so the rounds
    behind the static one draw from the M cursor."""
    size, n = 256, 600
    cams = [_camera(size, az) for az in (0.0, 2.0, -2.0, 4.0, -4.0, 6.0)]
    lengths, header = _run(oracle, _filling_scene(size, n), cams, size, True, plans, monkeypatch)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert (lengths == n).all() and int(header[7]) == 0 and int(header[6]) == len(lengths) > 4 * cus     # class_end[1], class_end[0]
