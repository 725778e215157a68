"""The forward blend's walk over the set bits of a wave's block (csrc/render_forward.hip) at the smallest shapes at which its
trip sizes and slot addresses can go wrong: 32 x 32 pixels (four tiles), at most 520 tiny Gaussians, sh_degree 0.

A wave owns one 8 x 4 pixel block of its tile and walks the entries whose alpha >= 1/255 region reaches that block, chunk
by chunk (64 list entries), two entries per pair: full trips of four pairs while more than four entries remain, then one
last trip of two pairs (3-4 left) or one pair (1-2 left).  Every scene here confines its Gaussians to single blocks
(tile 0's block 0 = columns 0-7, rows 0-3; block 7 = columns 8-15, rows 12-15), so the number of entries a wave walks in
each chunk is known, and is asserted on the CPU before anything runs on the GPU:
  * `_assert_on_cpu` takes the oracle's geometry and lists, evaluates the fork's alpha test in float64 at all 256 pixels of
    the tile for every entry, asserts the number of live entries of each block, and asserts that no (pixel, entry) alpha
    lies within KNIFE_EDGE (relative) of 1/255 and no tested transmittance within it of 1e-4 — so that expf and v_exp_f32
    cannot decide differently anywhere, and n_contrib must then equal the oracle's at EVERY pixel (no mismatch allowed);
  * images are held to IMG_TOL as everywhere (test_gpu_raster_parity._check_forward_scene).

The sums of a pixel are kept as two partial sums, one per lane half: the entries at even and at odd positions among the
live entries of the wave's block inside a chunk.  Entries of OTHER blocks move a block's entries to other slots of the
staged arrays and to other chunks (hence other trips), which must not change a bit as long as every entry keeps its
parity; `test_other_blocks_change_no_bit` builds its scenes so (asserted on the CPU) and says which entries move."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_bwd_pair_fold import _camera, _gaussians
from test_gpu_headline_parity import list_mode  # noqa: F401  (fixture)
from test_gpu_raster_parity import KNIFE_EDGE, _check_backward, _check_forward_scene, _dev, _oracle_forward, _settings

pytestmark = pytest.mark.gpu

H = W = 32
BG = (0.3, 0.1, 0.2)
ALPHA_MIN, T_MIN = 1.0 / 255.0, 1e-4


def _block_xy(rng, block, n):
    """Centres at least 2 pixels inside the 8 x 4 block (its pixels' coordinates are x0 .. x0 + 7, y0 .. y0 + 3)."""
    x0, y0 = (block & 1) * 8, (block >> 1) * 4
    return x0 + rng.uniform(1.5, 5.5, n), y0 + rng.uniform(1.45, 1.55, n)


@functools.lru_cache(maxsize=None)
def _scene(n0, n7=0, seed=0, opaque=0, where7=None):
    """n0 Gaussians in block 0 of tile 0 and n7 in block 7, all depths distinct; standard deviation 0.1-0.25 pixels before
    the rasterizer's 0.3 px^2 low-pass (about 0.6 pixels after it), opacity low enough that no pixel terminates.  The
    last `opaque` Gaussians of block 0 get opacity 0.99 and sit next to a pixel centre, behind all others, which then
    have opacity 0.02 and sit around the same pixel.  `where7`: ranks in
    depth order (among all n0 + n7) given to block 7's Gaussians; default: random.  Returns (scene, camera, block of each
    Gaussian in depth order)."""
    rng = np.random.default_rng(1000 * n0 + 10 * n7 + seed)
    cam = _camera(H, W)
    n = n0 + n7
    x0, y0 = _block_xy(rng, 0, n0)
    x7, y7 = _block_xy(rng, 7, n7)
    rank = rng.permutation(n)
    if where7 is not None:
        rest = np.setdiff1d(np.arange(n), np.asarray(where7))
        rank = np.concatenate([rest[rng.permutation(n0)], np.asarray(where7)])
    sigma = rng.uniform(0.1, 0.25, n)
    opacity = rng.uniform(0.8, 1.0, n) * min(0.3, 8.0 / max(n, 1))
    if opaque:
        # behind everything, a hundredth of a pixel off the centre of pixel (3, 2) (on it, power = 0 is a knife edge of its own):
        # alpha = 0.9898 there, so T = 0.87 -> 0.0089 -> 9e-5 < 1e-4 at the second of them; well below it one pixel away
        back = np.arange(n0 - opaque, n0)
        rank[back] = np.arange(n - opaque, n)
        front = np.setdiff1d(np.arange(n), back)
        rank[front] = np.argsort(np.argsort(rank[front]))
        x0[back], y0[back], sigma[back], opacity[back] = 3.01, 2.005, 0.1, 0.99
        x0[front], y0[front] = 3.0 + rng.uniform(-0.3, 0.3, front.size), 2.0 + rng.uniform(-0.05, 0.05, front.size)
        opacity[front] = 0.02
    z = 2.0 + 0.002 * rank
    sc = _gaussians(rng, cam, H, W, np.concatenate([x0, x7]), np.concatenate([y0, y7]), z, sigma, opacity, 0)
    block = np.concatenate([np.zeros(n0, int), np.full(n7, 7)])[np.argsort(rank)]
    return sc, cam, block


def _assert_on_cpu(oracle, sc, cam, live_per_block):
    """See the module docstring.  Returns (oracle object, its n_contrib image, block of every list entry of tile 0)."""
    ro, _ = _oracle_forward(oracle, sc, cam, H, W, BG, 0)
    keys, vals, ranges, tt, nc = ro.binning()
    geom = ro.geom()
    assert all(int(ranges[t, 1]) == int(ranges[t, 0]) for t in (1, 2, 3)), "only tile 0 has a list"
    ids = vals[int(ranges[0, 0]):int(ranges[0, 1])].astype(np.int64)
    assert ids.shape[0] == sum(live_per_block.values()) == sc["means3D"].shape[0], ids.shape
    co = geom["conic_opacity"][ids].astype(np.float64)
    m2 = geom["means2D"][ids].astype(np.float64)
    px = np.arange(16, dtype=np.float64)
    dx = m2[:, 0, None, None] - px[None, None, :]
    dy = m2[:, 1, None, None] - px[None, :, None]
    power = -0.5 * (co[:, 0, None, None] * dx * dx + co[:, 2, None, None] * dy * dy) - co[:, 1, None, None] * dx * dy
    a = np.minimum(0.99, co[:, 3, None, None] * np.exp(np.minimum(power, 0.0)))           # [entry, y, x]
    assert (np.abs(a / ALPHA_MIN - 1.0) >= KNIFE_EDGE).all(), "an alpha on the 1/255 knife edge: pick another seed"
    live = (power <= 0) & (a >= ALPHA_MIN)
    # blocks an entry is live in: exactly one, and each block has its intended number of entries
    in_block = np.stack([live[:, (b >> 1) * 4:(b >> 1) * 4 + 4, (b & 1) * 8:(b & 1) * 8 + 8].any((1, 2)) for b in range(8)], 1)
    assert (in_block.sum(1) == 1).all(), "a Gaussian reaches no block or two"
    assert {b: int(c) for b, c in enumerate(in_block.sum(0)) if c} == {b: c for b, c in live_per_block.items() if c}, in_block.sum(0)
    # the walk's transmittance tests, entry by entry (the fork's rule: an entry that would take T below 1e-4 ends the pixel)
    T = np.ones((16, 16))
    done = np.zeros((16, 16), bool)
    for e in range(ids.shape[0]):
        t = T * (1.0 - a[e])
        tested = live[e] & ~done
        assert (np.abs(t[tested] / T_MIN - 1.0) >= KNIFE_EDGE).all(), "a transmittance on the 1e-4 knife edge: pick another seed"
        stop = tested & (t < T_MIN)
        T = np.where(tested & ~stop, t, T)
        done |= stop
    assert float(ro.pixel_margins(np.arange(H * W)).min()) >= KNIFE_EDGE
    return ro, nc, np.argmax(in_block, 1)


def _forward(sc, cam):
    """(colour, depth, alpha, n_contrib, final_T) of one view."""
    import ctypes
    from gaussianip_amd import _lib
    from gaussianip_amd import rasterizer as R
    (color, radii, depth, alpha), plan = R.forward_with_state(
        _dev(sc["means3D"]), _dev(sc["opacities"]), [_settings(cam, H, W, BG, 0)], shs=_dev(sc["shs"]), scales=_dev(sc["scales"]),
        rotations=_dev(sc["rotations"]))
    torch.cuda.synchronize()
    n_contrib = R.state_views(plan)["n_contrib"][0].clone()
    layout, bucket_off = _lib.GipRasterStateLayout(), ctypes.c_size_t(0)
    assert _lib.raster_lib().gip_raster_state_layout_buckets(ctypes.byref(plan.cfg), int(getattr(plan, "bucket_stride", 0)),
                                                             ctypes.byref(layout), ctypes.byref(bucket_off)) == _lib.GIP_OK
    final_T = plan.state[layout.final_T:layout.final_T + 4 * H * W].view(torch.float32).reshape(H, W).clone()
    return color[0].clone(), depth[0].clone(), alpha[0].clone(), n_contrib, final_T


def _check(oracle, sc, cam, live_per_block):
    ro, nc, _ = _assert_on_cpu(oracle, sc, cam, live_per_block)
    _check_forward_scene(oracle, sc, cam, H, W, 0, bg=BG, nc_mismatch_frac=0.0)      # images at IMG_TOL, n_contrib equal everywhere
    return nc


@pytest.mark.parametrize("list_mode", ["culled", "exact"], indirect=True)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 16, 17, 20])
def test_every_tail_width_after_zero_one_and_two_full_trips(oracle, n, list_mode):
    sc, cam, _ = _scene(n)
    nc = _check(oracle, sc, cam, {0: n})
    assert int(nc.max()) == n, "the last entry contributes somewhere"


@pytest.mark.parametrize("list_mode", ["culled", "exact"], indirect=True)
@pytest.mark.parametrize("n", [63, 64, 65, 66, 71, 511, 512, 513, 515])
def test_chunk_and_batch_boundaries(oracle, n, list_mode):
    sc, cam, _ = _scene(n, seed={512: 1}.get(n, 0))      # seed 0 of the 512-entry scene has an alpha on the 1/255 knife edge
    nc = _check(oracle, sc, cam, {0: n})
    assert int(nc.max()) > n - 8, "the walk reaches the list's last trip"


@pytest.mark.parametrize("list_mode", ["culled", "exact"], indirect=True)
@pytest.mark.parametrize("n,where", [(9, "first slot of a 1-pair tail"), (10, "second slot of a 1-pair tail"),
                                     (12, "last pair of a 2-pair tail"), (11, "third slot of a 2-pair tail")])
def test_last_contributor_in_a_tail(oracle, n, where, list_mode):
    """One full trip, then the tail: the last entry of the list is the last contributor of some pixels."""
    sc, cam, _ = _scene(n, seed=3)
    ro, nc, _ = _assert_on_cpu(oracle, sc, cam, {0: n})
    assert int((nc == n).sum()) > 0, where
    got = _forward(sc, cam)[3].cpu().numpy().astype(np.uint32)
    assert np.array_equal(got, nc), where


@pytest.mark.parametrize("list_mode", ["culled", "exact"], indirect=True)
def test_termination_inside_a_tail(oracle, list_mode):
    """Eight entries of opacity 0.02 (one full trip), then three of 0.99 a hundredth of a pixel off one pixel centre (a 2-pair tail: two of them, then
    the third and a NULL slot).  At that pixel the second opaque entry takes T below 1e-4: it ends the pixel without
    contributing, and the third contributes nothing; one pixel away all three contribute."""
    sc, cam, _ = _scene(11, opaque=3)
    ro, nc, _ = _assert_on_cpu(oracle, sc, cam, {0: 11})
    assert int((nc == 9).sum()) > 0 and int((nc == 11).sum()) > 0, np.unique(nc)
    _check_forward_scene(oracle, sc, cam, H, W, 0, bg=BG, nc_mismatch_frac=0.0)


# Depth ranks, in the scene WITH the k added Gaussians, of block 7's Gaussians: first the two both scenes have (list
# positions 60 and 63 of the scene without the added ones: chunk 0 ends ... 0 7 0 0 7), then the added ones
RANKS7 = {1: (61, 64, 20), 3: (63, 66, 5, 20, 41), 7: (66, 69, 2, 9, 17, 20, 33, 41, 72)}


@pytest.mark.parametrize("k", [1, 3, 7])
def test_other_blocks_change_no_bit(oracle, k):
    """68 entries in block 0 and two in block 7 at list positions 60 and 63; then the same Gaussians with k more in block 7
    at interleaved depths.  Every entry of block 0 behind an added one moves to a later slot of the staged arrays.  k = 1
    pushes one of block 7's entries over the chunk boundary (block 0 keeps 62 + 6 entries per chunk, at other slots);
    k = 3 pushes two of block 0's entries into chunk 1 as well, and k = 7 (six in front of the boundary, one behind) four:
    the walk of chunk 0 then ends in another kind of last trip and every trip of chunk 1 holds other entries.  A pixel's
    sums are kept per lane half, i.e. per parity of an entry among its block's entries of the chunk, so equal bits can
    only be asked where every entry keeps its parity: an even number moves, from behind an even number that stays
    (asserted below on the oracle's lists).  Colour, depth and alpha of block 0's 32 pixels: equal bits."""
    full, cam, _ = _scene(68, 2 + k, seed=5, where7=RANKS7[k])
    base = {name: np.ascontiguousarray(v[:70]) for name, v in full.items()}
    ro_a, nc_a, blk_a = _assert_on_cpu(oracle, base, cam, {0: 68, 7: 2})
    ro_b, nc_b, blk_b = _assert_on_cpu(oracle, full, cam, {0: 68, 7: 2 + k})

    def walk_of_block0(blk):
        pos = np.flatnonzero(blk == 0)
        chunk = pos // 64
        rank_in_chunk = np.concatenate([np.arange(c) for c in np.bincount(chunk)])
        return pos, chunk, rank_in_chunk & 1
    pos_a, chunk_a, par_a = walk_of_block0(blk_a)
    pos_b, chunk_b, par_b = walk_of_block0(blk_b)
    assert [int(b) for b in blk_a[59:64]] == [0, 7, 0, 0, 7] and np.array_equal(par_a, par_b), "every entry of block 0 keeps its lane half"
    assert int((pos_a != pos_b).sum()) >= 20, "block 0's entries sit in other slots"
    assert int((chunk_a != chunk_b).sum()) == {1: 0, 3: 2, 7: 4}[k]
    a = _forward(base, cam)
    b = _forward(full, cam)
    for name, x, y in zip(("color", "depth", "alpha"), a[:3], b[:3]):
        assert torch.equal(x[..., 0:4, 0:8], y[..., 0:4, 0:8]), name
        assert float(x[..., 0:4, 0:8].abs().max()) > 0.0, name
    assert float(b[2][..., 12:16, 8:16].sum()) > float(a[2][..., 12:16, 8:16].sum()) > 0.0, "block 7 did change"


@pytest.mark.parametrize("n", [17, 71])
def test_forward_only_render_has_the_same_bits(n):
    from gaussianip_amd import rasterize_views
    sc, cam, _ = _scene(n)
    st = _settings(cam, H, W, BG, 0)

    def render(grad):
        t = {k: _dev(v).requires_grad_(grad) for k, v in sc.items()}
        with (torch.enable_grad() if grad else torch.no_grad()):
            out = rasterize_views(t["means3D"], None, t["opacities"], [st], shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
        torch.cuda.synchronize()
        return out
    with_state, without = render(True), render(False)
    assert with_state[0].requires_grad and not without[0].requires_grad
    for x, y in zip(with_state, without):
        assert torch.equal(x.detach(), y) and float(y.float().abs().max()) > 0.0


@pytest.mark.parametrize("list_mode", ["culled", "exact"], indirect=True)
@pytest.mark.parametrize("n0,n7", [(71, 0), (67, 4)])
def test_backward_parity_behind_a_checkpoint(oracle, n0, n7, list_mode):
    """71 list entries: the second segment's checkpoint is written after chunk 0.  (71, 0): chunk 0 is eight full trips of
    wave 0.  (67, 4): four of the first 64 entries belong to block 7, so wave 0's chunk 0 ends in a 2-pair tail (60
    entries) and wave 7 walks nothing but one."""
    sc, cam, _ = _scene(n0, n7, where7=(3, 19, 40, 58) if n7 else None)
    ro, nc, blk = _assert_on_cpu(oracle, sc, cam, {0: n0, 7: n7})
    if n7:
        assert int((blk[:64] == 0).sum()) == 60
    _check_backward(oracle, "tail trips", n0 + n7, H, W, 7, 0, scene=dict(sc), cam=cam, bg=BG)


def test_two_runs_give_equal_bits():
    sc, cam, _ = _scene(71)
    a, b = _forward(sc, cam), _forward(sc, cam)
    for x, y in zip(a, b):
        assert torch.equal(x, y) and float(x.float().abs().max()) > 0.0
