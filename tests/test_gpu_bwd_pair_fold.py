"""The backward blend's two-entries-per-trip walk (csrc/render_backward.hip: fold_two_entries) at the smallest shapes at
which it can go wrong: 32 x 32 pixels (four tiles), at most 130 Gaussians, sh_degree 0 or 1.

The kernel takes the live entries of a 64-entry segment two at a time, reduces both entries' ten terms with one cross-lane
fold and stores each entry's row from the lanes that hold its sums.  What can go wrong there and what pins it here:
  * the odd tail (an entry paired with an all-zero partner that has no row), a pair that ends a segment and a lone entry
    that opens the next one: tiles with 1, 2, 3, 63, 64, 65 and 129 live entries, against the CPU oracle at
    test_gpu_raster_parity._check_backward's bars (2e-3 of the tensor maximum with the backward isolated, unchanged);
  * entries whose quadrant mask is zero (they are skipped by the walk and their row is zeroed by the lane that staged
    them) and one such dead entry BETWEEN two live ones, which GIP_RASTER_EXACT_LISTS=1 keeps in the lists: a Gaussian of
    opacity 0.006 one and a half pixels from a tile border, whose 3-sigma rectangle reaches the neighbouring tile and whose
    alpha >= 1/255 region does not.  The oracle's binning() and a brute-force alpha test over the tile's 256 pixels
    assert these list lengths and live counts on the CPU before anything runs on the GPU;
  * a capacity hint smaller than the scene's instance count (rows beyond the capacity): the forward flags the overflow,
    the step must come out as exact zeros with the usual warning, and the next call must give the usual gradients again;
  * an entry's row must not depend on its slot in the pair nor on its partner: one more Gaussian in the diagonally opposite
    quadrant of a single tile, nearest in depth, moves every subject to the other slot, and the subjects' gradients must
    not change by one bit;
  * run to run, equal bits."""
import functools

import numpy as np
import pytest
import torch

import scenes
from scenes import gaussians_at_pixels as _gaussians  # noqa: F401  (test_gpu_fwd_tail_trips.py imports it from here)
from test_gpu_headline_parity import list_mode  # noqa: F401  (fixture)
from test_gpu_raster_parity import _check_backward, _dev, _oracle_forward, _settings

pytestmark = pytest.mark.gpu

H = W = 32
BG = (0.3, 0.1, 0.2)
GRADS = ("means3D", "opacities", "shs", "scales", "rotations")
DEAD_OPACITY = 0.006
# name -> (live entries of tiles 0..3 (the border Gaussian counted in its own tile), tile of the border Gaussian, the
#          neighbouring tile its 3-sigma rectangle reaches, sh_degree)
SCENES = {
    "1-2-3-63": ((1, 2, 3, 63), 0, 1, 0),
    "64-65": ((64, 65, 0, 0), 0, 1, 1),
    "129-1": ((129, 1, 0, 0), 1, 0, 1),
}


def _camera(h, w):
    return scenes.camera(0.0, 0.0, 2.0, 50.0, h, w)


@functools.lru_cache(maxsize=None)
def _build(name):
    """Scene of the table above.  Regular Gaussians: centres 4.5-11.5 pixels inside their tile and at most 1.2 pixels wide
    (3-sigma radius <= 4: the rectangle stays inside the tile), opacity 0.05-0.3, all depths distinct.  Returns
    (scene, camera, index of the border Gaussian)."""
    live, border_tile, reached_tile, deg = SCENES[name]
    rng = np.random.default_rng(sum(live))
    cam = _camera(H, W)
    tile = np.concatenate([np.full(n - (t == border_tile), t) for t, n in enumerate(live)])
    n = tile.shape[0]
    px = (tile % 2) * 16 + rng.uniform(4.5, 11.5, n)
    py = (tile // 2) * 16 + rng.uniform(4.5, 11.5, n)
    z = 2.0 + 0.002 * rng.permutation(n + 1)[:n]
    # the border Gaussian: 1.5 pixels from the border to `reached_tile`, in depth between that tile's entries
    zr = np.sort(z[tile == reached_tile])
    zb = 0.5 * (zr[0] + zr[1]) if zr.shape[0] >= 2 else 2.0 + 0.002 * n
    bx = 14.5 if border_tile < reached_tile else 17.5
    px, py, z = np.append(px, bx), np.append(py, 8.0), np.append(z, zb)
    sigma = np.append(rng.uniform(0.6, 1.2, n), 1.0)
    opacity = np.append(rng.uniform(0.05, 0.3, n), DEAD_OPACITY)
    sc = _gaussians(rng, cam, H, W, px, py, z, sigma, opacity, deg)
    # the border Gaussian is isotropic: its reach is the one worked out in the module docstring
    sc["scales"][n] = sc["scales"][n].max()
    return sc, cam, n


def _alive(geom, g, x0, y0):
    """Does Gaussian g pass the alpha >= 1/255 test at any of the 256 pixels of the tile at (x0, y0)?  (float64 evaluation of
    the fork's test, as test_gpu_raster_parity.compare_tile_lists does it)"""
    return bool(_alpha_region(geom, g, x0, y0, 16, 16).any())


def _alpha_region(geom, g, x0, y0, h, w):
    co = geom["conic_opacity"][g].astype(np.float64)
    dx = float(geom["means2D"][g, 0]) - (x0 + np.arange(w, dtype=np.float64))[None, :]
    dy = float(geom["means2D"][g, 1]) - (y0 + np.arange(h, dtype=np.float64))[:, None]
    power = -0.5 * (co[0] * dx * dx + co[2] * dy * dy) - co[1] * dx * dy
    return (power <= 0) & (np.minimum(0.99, co[3] * np.exp(np.minimum(power, 0.0))) >= 1.0 / 255.0)


def _assert_lists_on_cpu(oracle, name):
    """The oracle's (= the fork's 3-sigma) lists of the scene: every tile has its live entries and nothing else, except the
    reached tile, which has the border Gaussian's dead entry as well — between two live ones where the tile has two."""
    sc, cam, border = _build(name)
    live, border_tile, reached_tile, deg = SCENES[name]
    ro, _ = _oracle_forward(oracle, sc, cam, H, W, BG, deg)
    keys, vals, ranges, tt, nc = ro.binning()
    geom = ro.geom()
    for t in range(4):
        ids = vals[int(ranges[t, 0]):int(ranges[t, 1])].astype(np.int64)
        alive = np.array([_alive(geom, g, (t % 2) * 16, (t // 2) * 16) for g in ids], dtype=bool)
        assert int(alive.sum()) == live[t], (name, t, int(alive.sum()))
        assert ids.shape[0] == live[t] + (t == reached_tile), (name, t, ids.shape[0])
        if t == reached_tile:
            dead = np.flatnonzero(~alive)
            assert dead.shape[0] == 1 and ids[dead[0]] == border, (name, ids[dead])
            if live[t] >= 2:
                assert alive[:dead[0]].any() and alive[dead[0] + 1:].any(), "the dead entry sits between live ones"
    # every pixel's walk stays open to the end of its list (no early termination shortens what the backward replays)
    assert int(nc.max()) > 0
    return sum(live), sum(live) + 1


def _library_num_rendered(sc, cam, h, w, deg):
    from gaussianip_amd import rasterizer as R
    _, plan = R.forward_with_state(_dev(sc["means3D"]), _dev(sc["opacities"]), [_settings(cam, h, w, BG, deg)], shs=_dev(sc["shs"]),
                                   scales=_dev(sc["scales"]), rotations=_dev(sc["rotations"]))
    torch.cuda.synchronize()
    hdr = R.state_views(plan)["header"].cpu().numpy()
    assert int(hdr[2]) == 0, "overflow"
    return int(hdr[1])


def _upstream(seed, h, w):
    rng = np.random.default_rng(seed)
    return tuple(_dev(rng.normal(size=(c, h, w)).astype(np.float32)) for c in (3, 1, 1))


def _grads(sc, cam, h, w, deg, up):
    """Forward + backward of one view; {name: gradient} as torch tensors on the device."""
    from gaussianip_amd import GaussianRasterizer
    t = {k: _dev(v).requires_grad_(True) for k, v in sc.items()}
    m2 = torch.zeros(sc["means3D"].shape[0], 3, device="cuda", requires_grad=True)
    color, radii, depth, alpha = GaussianRasterizer(_settings(cam, h, w, BG, deg))(
        means3D=t["means3D"], means2D=m2, opacities=t["opacities"], shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    g = torch.autograd.grad([color, depth, alpha], [t[k] for k in GRADS] + [m2], list(up))
    torch.cuda.synchronize()
    return dict(zip(GRADS + ("means2D",), g))


@pytest.mark.parametrize("list_mode", ["culled", "exact"], indirect=True)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_backward_parity_on_pair_edge_cases(oracle, name, list_mode):
    sc, cam, border = _build(name)
    deg = SCENES[name][3]
    n_live, n_listed = _assert_lists_on_cpu(oracle, name)
    # the library walked these lists: the default mode drops the dead entry, exact lists keep it
    assert _library_num_rendered(sc, cam, H, W, deg) == (n_listed if list_mode == "exact" else n_live)
    _check_backward(oracle, "pair edge cases", sc["means3D"].shape[0], H, W, 7, deg, scene=dict(sc), cam=cam, bg=BG)


def test_rows_beyond_the_capacity_give_a_zero_step_and_the_next_call_recovers():
    from gaussianip_amd import rasterizer as R
    sc, cam, border = _build("129-1")
    deg = SCENES["129-1"][3]
    P = sc["means3D"].shape[0]
    up = _upstream(3, H, W)
    ref = _grads(sc, cam, H, W, deg, up)
    key = R._hint_key(torch.device("cuda", torch.cuda.current_device()), P, 1, H, W)
    assert R._capacity_hint[key] == 130
    old = R._MIN_CAPACITY, R._CAPACITY_MARGIN
    try:
        R._MIN_CAPACITY, R._CAPACITY_MARGIN = 64, 0
        R._capacity_hint[key] = 20                  # capacity 64: the rows of 66 of the 130 instances lie beyond it
        with pytest.warns(RuntimeWarning, match="exceeded the capacity hint"):
            zero = _grads(sc, cam, H, W, deg, up)
        for k, v in zero.items():
            assert bool(torch.isfinite(v).all()) and float(v.abs().max()) == 0.0, k
        again = _grads(sc, cam, H, W, deg, up)      # capacity 3 x 130 now
        for k in ref:
            assert torch.equal(again[k], ref[k]) and float(ref[k].abs().max()) > 0.0, k
    finally:
        R._MIN_CAPACITY, R._CAPACITY_MARGIN = old


def test_a_row_does_not_depend_on_the_pair_slot_or_the_partner(oracle):
    """One 16 x 16 tile, 37 subjects whose alpha >= 1/255 regions lie in the upper left quadrant, then the same with one more
    Gaussian in the lower right quadrant in front of them all: it becomes entry 0 of the list, so every subject changes
    its slot in the pair and its partner."""
    h = w = 16
    n, deg = 37, 1
    rng = np.random.default_rng(11)
    cam = _camera(h, w)
    px = np.append(rng.uniform(2.5, 4.6, n), 12.0)
    py = np.append(rng.uniform(2.5, 4.6, n), 12.0)
    z = np.append(2.0 + 0.002 * (1 + rng.permutation(n)), 2.0)
    both = _gaussians(rng, cam, h, w, px, py, z, np.full(n + 1, 0.58), np.append(rng.uniform(0.05, 0.3, n), 0.5), deg)
    subjects = {k: np.ascontiguousarray(v[:n]) for k, v in both.items()}
    # on the CPU: the extra Gaussian is the nearest, its alpha >= 1/255 region shares no pixel with any subject's, and one
    # tile's list holds them all
    ro, _ = _oracle_forward(oracle, both, cam, h, w, BG, deg)
    geom = ro.geom()
    keys, vals, ranges, tt, nc = ro.binning()
    assert ranges.shape[0] == 1 and int(ranges[0, 1]) - int(ranges[0, 0]) == n + 1 < 64 and int(vals[0]) == n
    region = np.stack([_alpha_region(geom, g, 0, 0, h, w) for g in range(n + 1)])
    assert region[n].any() and region[:n].any((1, 2)).all() and not (region[n] & region[:n].any(0)).any()
    assert not region[:n, 8:, :].any() and not region[:n, :, 8:].any() and not region[n, :8, :].any() and not region[n, :, :8].any()
    up = _upstream(5, h, w)
    alone = _grads(subjects, cam, h, w, deg, up)
    shifted = _grads(both, cam, h, w, deg, up)
    for k in GRADS:
        assert float(alone[k].abs().max()) > 0.0 and float(shifted[k][n].abs().max()) > 0.0, k
        assert torch.equal(alone[k], shifted[k][:n]), k


@pytest.mark.parametrize("list_mode", ["culled", "exact"], indirect=True)
def test_backward_on_pair_edge_cases_is_bitwise_reproducible(list_mode):
    for name in sorted(SCENES):
        sc, cam, border = _build(name)
        deg = SCENES[name][3]
        up = _upstream(9, H, W)
        a = _grads(sc, cam, H, W, deg, up)
        b = _grads(sc, cam, H, W, deg, up)
        for k in a:
            assert torch.equal(a[k], b[k]), (name, k)
            assert bool(torch.isfinite(a[k]).all()) and float(a[k].abs().max()) > 0.0, (name, k)
