"""Volume rendering without a GPU (csrc/volume.hip, gaussianip_amd/utils/volume.py): the float64 restatement's analytic gradients
against central differences, the float32 op chain against the restatement, the march restatement on rays that can be checked by hand,
the occupancy grid's update and the pruning mask on CPU tensors, the implicit volume's density bias and activation, the ray helpers,
the exported symbols, the entry points' argument checks (which launch nothing), the share of undecided samples in the GPU pruning test's
inputs and the compiler's resource report of every kernel of the file."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import volume_inputs as inputs
import volume_reference as reference
from test_model_no_spills_cpu import HIPCC, resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("volume_march_count_kernel", "volume_march_emit_kernel", "volume_weights_forward_kernel", "volume_weights_backward_kernel",
           "volume_accumulate_forward_kernel", "volume_accumulate_backward_kernel")
SYMBOLS = ["gip_volume_march_count", "gip_volume_march_emit", "gip_volume_weights_forward", "gip_volume_weights_backward",
           "gip_volume_accumulate_forward", "gip_volume_accumulate_backward"]


def test_symbols_exported():
    from gaussianip_amd import _lib
    from gaussianip_amd.scene import GaussianModel
    from gaussianip_amd.utils import volume
    so = os.path.join(ROOT, "gaussianip_amd", "lib", "libgip_model.so")
    assert os.path.exists(so), "libgip_model.so is not built"
    names = {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout.splitlines()
             if ln.strip()}
    lib = _lib.model_lib()
    with open(os.path.join(ROOT, "include", "gip_model.h")) as fh:
        header = fh.read()
    assert _lib.VOLUME_SYMBOLS == SYMBOLS
    for sym in SYMBOLS:
        assert sym in names and getattr(lib, sym) is not None and "int %s(" % sym in header, sym
    with open(os.path.join(ROOT, "gaussianip_amd", "csrc", "Makefile")) as fh:
        assert fh.read().count("volume.hip") == 2                    # a prerequisite of libgip_model.so and a source of its command
    assert volume.__all__ == ["march_rays", "render_weight_from_density", "accumulate_along_rays", "OccupancyGrid", "ImplicitVolume",
                              "NeRFVolumeRenderer", "get_ray_directions", "get_rays"]
    assert callable(GaussianModel.render_field_volume)


# ---------------------------------------------------------------------------------------------------------------- the march, by hand
def _hand_case(occ_cells, o, d, **over):
    occ = np.zeros((2, 2, 2), np.uint8)
    for c in occ_cells:
        occ[c] = 1
    case = dict(rays_o=np.array([o], np.float32), rays_d=np.array([d], np.float32), occ=occ, lo=np.full(3, -1, np.float32),
                hi=np.full(3, 1, np.float32), scale=np.full(3, 1, np.float32), dt=0.5, near=0.0, far=1e10, jitter=None, K_cap=1024)
    case.update(over)
    return case


def test_march_restatement_on_hand_checked_rays():
    # along +x at y = z = -0.5 through a 2^3 grid over [-1, 1]^3: in at t = 1, out at t = 3, four steps of 0.5 with midpoints at
    # x = -0.75, -0.25, 0.25, 0.75, that is two in cell (0, 0, 0) and two in cell (1, 0, 0)
    o, d = (-2.0, -0.5, -0.5), (1.0, 0.0, 0.0)
    idx, ts, te, off = reference.march(_hand_case([(0, 0, 0)], o, d))
    assert idx.tolist() == [0, 0] and ts.tolist() == [1.0, 1.5] and te.tolist() == [1.5, 2.0] and off.tolist() == [0, 2]
    assert idx.dtype == off.dtype == np.int32 and ts.dtype == te.dtype == np.float32
    idx, ts, te, off = reference.march(_hand_case([(1, 0, 0)], o, d))
    assert ts.tolist() == [2.0, 2.5] and te.tolist() == [2.5, 3.0]
    idx, ts, te, off = reference.march(_hand_case([(0, 0, 0), (1, 0, 0)], o, d))
    assert ts.tolist() == [1.0, 1.5, 2.0, 2.5] and te.tolist() == [1.5, 2.0, 2.5, 3.0]
    # the other cells of the row are not read: the same ray at y = z = +0.5 walks cells (., 1, 1)
    assert reference.march(_hand_case([(0, 0, 0), (1, 0, 0)], (-2.0, 0.5, 0.5), d))[0].size == 0
    assert reference.march(_hand_case([(0, 1, 1)], (-2.0, 0.5, 0.5), d))[1].tolist() == [1.0, 1.5]
    # half a step of jitter: the last interval is cut at the exit
    full = [(0, 0, 0), (1, 0, 0)]
    idx, ts, te, off = reference.march(_hand_case(full, o, d, jitter=np.array([0.5], np.float32)))
    assert ts.tolist() == [1.25, 1.75, 2.25, 2.75] and te.tolist() == [1.75, 2.25, 2.75, 3.0]
    # near and far cut the span; K_cap cuts the candidates
    assert reference.march(_hand_case(full, o, d, near=1.75))[1].tolist() == [1.75, 2.25, 2.75]
    idx, ts, te, off = reference.march(_hand_case(full, o, d, far=2.25))
    assert ts.tolist() == [1.0, 1.5, 2.0] and te.tolist() == [1.5, 2.0, 2.25]
    assert reference.march(_hand_case(full, o, d, K_cap=3))[1].tolist() == [1.0, 1.5, 2.0]
    # the miss: above the box; behind the origin; touching a corner only (t_near == t_far)
    assert reference.march(_hand_case(full, (-2.0, 1.5, 0.0), (1.0, 0.1, 0.0)))[0].size == 0
    assert reference.march(_hand_case(full, (2.0, -0.5, -0.5), d))[0].size == 0
    assert reference.march(_hand_case(full, (-3.0, 1.0, -0.5), (1.0, -1.0, 0.0)))[0].size == 0
    # the zero-direction axis gives no bounds and decides by lo <= o <= hi alone, the faces included
    assert reference.ray_span((-2.0, 1.0, -1.0), d, *_box()) == (1.0, 3.0)
    assert reference.ray_span((-2.0, 1.0000001, 0.0), d, *_box()) is None
    assert reference.ray_span((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), *_box()) is None
    assert reference.ray_span((0.0, 0.0, 0.0), (0.0, 0.0, -2.0), *_box()) == (0.0, 0.5)
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert reference.ray_span((bad, 0.0, 0.0), d, *_box()) is None and reference.ray_span(o, (1.0, bad, 0.0), *_box()) is None


def _box():
    return np.full(3, -1, np.float32), np.full(3, 1, np.float32), 0.0, 1e10


def test_the_trip_case_has_the_counts_it_names():
    ray_indices, t_starts, t_ends, offsets = inputs.marched("trips")
    counts = np.diff(offsets)
    assert tuple(counts[:len(inputs.TRIP_COUNTS)]) == inputs.TRIP_COUNTS and counts[len(inputs.TRIP_COUNTS):].min() > 64
    assert (np.diff(ray_indices) >= 0).all() and ray_indices.shape[0] == offsets[-1]
    for name in inputs.MARCH_CASES:
        idx, ts, te, off = inputs.marched(name)
        case = inputs.march_case(name)
        assert off.shape[0] == case["rays_o"].shape[0] + 1 and off[-1] == idx.shape[0] and (ts < te).all()
        inside = np.repeat(np.diff(off) > 0, np.diff(off))
        assert inside.all()
        same_ray = idx[1:] == idx[:-1]
        assert (ts[1:][same_ray] > ts[:-1][same_ray]).all()          # ordered by t inside a ray
    assert inputs.marched("d_zeros")[0].size == 0 and inputs.marched("e_r0")[0].size == 0
    edge = np.diff(inputs.marched("d_ones")[3])
    what = [r[2] for r in inputs.EDGE_RAYS]
    for label, hit in (("origin inside the box", True), ("one zero component, outside its slab", False), ("a miss", False),
                       ("origin exactly on a face, pointing in", True), ("origin exactly on a face, pointing out", False),
                       ("NaN origin", False), ("infinite direction", False), ("zero direction, inside the box", False),
                       ("a denormal component: 1 / d is infinite", True)):
        assert (edge[what.index(label)] > 0) == hit, label
    assert np.diff(inputs.marched("d_kcap")[3]).max() == 10 and (np.diff(inputs.marched("d_far")[3]) <= edge).all()
    assert inputs.marched("d_far")[2].max() == np.float32(2.5)


# ---------------------------------------------------------------------------------------------------------------- compositing
def _central(fn, x, g, h=1e-6):
    """d sum(fn(x) * g) / d x by central differences in float64."""
    out = np.zeros_like(x)
    flat, view = x.reshape(-1), out.reshape(-1)
    for i in range(flat.shape[0]):
        keep = flat[i]
        flat[i] = keep + h
        up = (fn(x) * g).sum()
        flat[i] = keep - h
        down = (fn(x) * g).sum()
        flat[i] = keep
        view[i] = (up - down) / (2 * h)
    return out


def test_analytic_gradients_against_central_differences():
    rng = np.random.default_rng(7)
    offsets = np.array([0, 0, 5, 6, 6, 17], np.int32)                # an empty ray first, a one-sample ray, an empty one between
    M = 17
    ray_indices = np.repeat(np.arange(5), np.diff(offsets))
    ts = np.sort(rng.random(M)) * 3
    te = ts + rng.random(M) * 0.2 + 0.01
    sigmas, g_w = rng.random(M) * 20, rng.standard_normal(M)
    analytic = reference.weights_backward_f64(ts, te, sigmas, offsets, g_w)
    numeric = _central(lambda s: reference.weights_f64(ts, te, s, offsets)[0], sigmas.copy(), g_w)
    assert np.abs(analytic - numeric).max() <= 1e-7 * np.abs(analytic).max()
    w = reference.weights_f64(ts, te, sigmas, offsets)[0]
    for C in (1, 3):
        v, g_out = rng.standard_normal((M, C)), rng.standard_normal((5, C))
        g_wa, g_va = reference.accumulate_backward_f64(w, v, ray_indices, g_out)
        assert np.abs(g_wa - _central(lambda x: reference.accumulate_f64(x, v, offsets), w.copy(), g_out)).max() <= 1e-8
        assert np.abs(g_va - _central(lambda x: reference.accumulate_f64(w, x, offsets), v.copy(), g_out)).max() <= 1e-8
    g_out = rng.standard_normal((5, 1))
    g_wa, g_va = reference.accumulate_backward_f64(w, None, ray_indices, g_out)
    assert np.allclose(g_wa, g_out[ray_indices, 0]) and np.array_equal(reference.accumulate_f64(w, None, offsets)[:, 0],
                                                                      reference.accumulate_f64(w, np.ones((M, 1)), offsets)[:, 0])
    # a ray index outside [0, R) contributes nothing
    g_wa, g_va = reference.accumulate_backward_f64(w, None, np.where(ray_indices == 2, 99, ray_indices), g_out)
    assert g_wa[5] == 0 and g_va[5, 0] == 0 and g_wa[0] == g_out[1, 0]
    # transmittance restarts at every ray, the weights of a ray sum to 1 - its final transmittance
    w, trans, alphas = reference.weights_f64(ts, te, sigmas, offsets)
    assert (trans[offsets[:-1][np.diff(offsets) > 0]] == 1).all()
    opacity = reference.accumulate_f64(w, None, offsets)[:, 0]
    assert opacity[0] == 0 and np.allclose(opacity[4], 1 - trans[16] * (1 - alphas[16]))


def test_op_chain_against_the_restatement():
    c = inputs.composite()
    f64, w_acc = reference.composite_f64(c)
    # float32: the chain's cumsum runs over all M = 3155 samples and reaches S of about 600, so a ray's sum, a difference of two of its
    # values, carries about sqrt(M) x 2^-24 x S = 2e-3 of rounding (a random walk; the worst case is M x 2^-24 x S), and exp() hands
    # that on to trans and the weights as a relative error.  The kernels sum inside a ray only.  The accumulate sums 300 terms a ray.
    for dtype, tol_weights, tol_accumulate in ((torch.float64, 1e-12, 1e-12), (torch.float32, 2e-3, 300 * 2.0 ** -24)):
        chained = reference.Chained(dtype)
        chain = reference.composite_run(c, w_acc, chained.render_weight_from_density, chained.accumulate_along_rays, dtype=dtype)
        assert sorted(chain) == sorted(f64)
        for name, truth in f64.items():
            tol = tol_weights if name in ("weights", "trans", "alphas", "g_sigmas") else tol_accumulate
            assert chain[name].shape == truth.shape and np.abs(chain[name] - truth).max() <= tol * np.abs(truth).max(), (name, dtype)


# ---------------------------------------------------------------------------------------------------------------- pruning
def test_few_pruning_samples_are_undecided():
    """The GPU pruning test lets a sample go either way when, in float64, |alpha - alpha_thre| <= 1e-5 or |trans - early_stop_eps| <=
    1e-4 early_stop_eps (float32 rounding over at most 512 summed terms is about 3e-5 relative in the worst case): on its inputs at
    most 1 % of the samples are that close, and both outcomes occur among the rest."""
    p = inputs.pruning()
    _, trans, alphas = reference.weights_f64(p["t_starts"], p["t_ends"], p["sigmas"], p["offsets"])
    undecided = (np.abs(alphas - inputs.ALPHA_THRE) <= 1e-5) | (np.abs(trans - inputs.EARLY_STOP_EPS) <= 1e-4 * inputs.EARLY_STOP_EPS)
    keep = (alphas >= inputs.ALPHA_THRE) & (trans >= inputs.EARLY_STOP_EPS)
    M = trans.shape[0]
    print("pruning inputs: %d samples, %d undecided, %d kept" % (M, int(undecided.sum()), int(keep.sum())))
    assert M > 5000 and undecided.sum() <= 0.01 * M
    assert (alphas < inputs.ALPHA_THRE).sum() > 100 and (trans < inputs.EARLY_STOP_EPS).sum() > 100 and 100 < keep.sum() < M - 100


def test_prune_mask_and_occupancy_grid_on_cpu_tensors():
    from gaussianip_amd.utils.volume import OccupancyGrid, prune_mask
    trans = torch.tensor([1.0, 0.5, 1e-4, 0.99e-4, 0.3])
    alphas = torch.tensor([0.01, 0.0099, 0.5, 0.5, 0.0])
    assert prune_mask(trans, alphas, 0.01, 1e-4).tolist() == [True, False, True, False, False]
    assert prune_mask(trans, alphas, 0.0, 0.0).all()

    grid = OccupancyGrid([-1, -1, -1, 1, 1, 1], resolution=8)
    assert grid.occs.shape == (512,) and grid.binaries.shape == (8, 8, 8) and grid.binaries.dtype == torch.bool and not grid.binaries.any()
    asked = []

    def ball(x):                                                     # 1 inside the ball of radius 0.5, else 0
        asked.append(x)
        return ((x * x).sum(-1, keepdim=True) < 0.25).float()
    torch.manual_seed(0)
    grid.update_every_n_steps(3, ball)                               # not an n-th step
    assert not asked
    grid.update_every_n_steps(0, ball)
    (x,) = asked
    assert x.shape == (512, 3)                                       # warm-up: every cell, one point inside each
    cell = torch.floor((x + 1) / 2 * 8).long()
    assert torch.equal((cell[:, 0] * 8 + cell[:, 1]) * 8 + cell[:, 2], torch.arange(512))
    centres = (torch.stack(torch.meshgrid(*(torch.arange(8),) * 3, indexing="ij"), -1).float() + 0.5) / 4 - 1
    far = centres.norm(dim=-1) > 0.5 + 0.25 * 3 ** 0.5
    near = centres.norm(dim=-1) < 0.5 - 0.25 * 3 ** 0.5
    assert not grid.binaries[far].any() and grid.binaries[near].all() and 0 < int(grid.binaries.sum()) < 512
    assert torch.equal(grid.binaries.reshape(-1), grid.occs > min(float(grid.occs.mean()), 0.01))
    before, occupied = grid.occs.clone(), int(grid.binaries.sum())
    grid.update_every_n_steps(256, lambda x: torch.zeros(x.shape[0]), warmup_steps=256)      # after warm-up: a quarter + the occupied cells
    touched = grid.occs != before
    assert torch.equal(grid.occs[touched], before[touched] * 0.95) and not (touched & (before == 0)).any()
    assert int(touched.sum()) == occupied                            # every occupied cell was asked and decayed; empty ones stay 0
    for _ in range(100):                                             # the occupied cells are asked every time: 0.95^101 < 0.01
        grid.update_every_n_steps(256, lambda x: torch.zeros(x.shape[0]), warmup_steps=0)
    assert float(grid.occs.max()) < 0.01
    with pytest.raises(ValueError):
        OccupancyGrid([-1, -1, -1, 1, 1, 1], resolution=0)
    with pytest.raises(ValueError):
        OccupancyGrid([-1, -1, -1, 1, -1, 1])
    with pytest.raises(ValueError, match="float32 GPU"):
        grid.sampling(torch.zeros(4, 3), torch.ones(4, 3), render_step_size=0.1)


# ---------------------------------------------------------------------------------------------------------------- geometry and rays
SMALL_GRID = {"otype": "HashGrid", "n_levels": 2, "n_features_per_level": 2, "log2_hashmap_size": 6, "base_resolution": 4, "per_level_scale": 1.5}


def test_implicit_volume_density_bias_and_activation():
    from gaussianip_amd.utils.volume import ImplicitVolume
    pts = torch.tensor([[0.0, 0.0, 0.0], [0.3, -0.4, 0.0], [1.0, 1.0, 1.0]], dtype=torch.float64)
    net = torch.tensor([[0.5], [-2.0], [1.0]], dtype=torch.float64)
    r = pts.norm(dim=-1, keepdim=True)
    cases = (("blob_magic3d", 10.0 * (1 - r / 0.5)), ("blob_dreamfusion", 10.0 * torch.exp(-0.5 * r ** 2 / 0.25)), (-1.5, torch.full_like(r, -1.5)))
    acts = {"softplus": torch.nn.functional.softplus, "exp": torch.exp, "relu": torch.relu, "none": lambda x: x}
    for bias, expected in cases:
        for act, fn in acts.items():
            vol = ImplicitVolume(radius=1.0, density_bias=bias, density_activation=act, pos_encoding_config=SMALL_GRID)
            raw, density = vol.get_activated_density(pts, net)
            assert torch.allclose(raw, net + expected, rtol=1e-12, atol=0) and torch.equal(density, fn(raw)), (bias, act)
    vol = ImplicitVolume(radius=2.0, n_feature_dims=5, normal_type="pred", pos_encoding_config=SMALL_GRID)
    assert vol.bbox.tolist() == [[-2.0] * 3, [2.0] * 3] and vol.feature_network.layers[-1].out_features == 5
    assert torch.equal(vol._unit(vol.bbox), torch.tensor([[0.0] * 3, [1.0] * 3]))
    assert vol.normal_network.layers[-1].out_features == 3 and vol.density_network.layers[-1].out_features == 1
    assert not hasattr(ImplicitVolume(n_feature_dims=0, normal_type=None, pos_encoding_config=SMALL_GRID), "feature_network")
    for bad in (dict(normal_type="analytic"), dict(density_bias="blob"), dict(density_activation="sigmoid"), dict(radius=0.0)):
        with pytest.raises(ValueError):
            ImplicitVolume(pos_encoding_config=SMALL_GRID, **bad)


def test_get_rays_against_a_hand_built_camera():
    from gaussianip_amd.utils.volume import get_ray_directions, get_rays
    dirs = get_ray_directions(2, 4, 2.0)
    assert dirs.shape == (2, 4, 3)
    # pixel centres at columns 0.5 .. 3.5 about cx = 2 and rows 0.5, 1.5 about cy = 1, focal 2; y up, looking along -z
    assert dirs[..., 0].tolist() == [[-0.75, -0.25, 0.25, 0.75]] * 2
    assert dirs[..., 1].tolist() == [[0.25] * 4, [-0.25] * 4] and (dirs[..., 2] == -1).all()
    assert get_ray_directions(2, 4, 2.0, use_pixel_centers=False)[0, 0].tolist() == [-1.0, 0.5, -1.0]
    assert get_ray_directions(2, 4, (2.0, 4.0), principal=(1.0, 0.5))[1, 3].tolist() == [1.25, -0.25, -1.0]
    with pytest.raises(ValueError):
        get_ray_directions(2, 4, (2.0, 4.0))
    # a camera at (1, 2, 3) turned a quarter about y: its -z axis (the view direction) is the world's -x
    c2w = torch.tensor([[0.0, 0.0, 1.0, 1.0], [0.0, 1.0, 0.0, 2.0], [-1.0, 0.0, 0.0, 3.0], [0.0, 0.0, 0.0, 1.0]])
    rays_o, rays_d = get_rays(dirs, c2w, keepdim=True)
    assert rays_o.shape == rays_d.shape == (2, 4, 3) and (rays_o == torch.tensor([1.0, 2.0, 3.0])).all()
    expect = torch.stack((-torch.ones(2, 4), dirs[..., 1], -dirs[..., 0]), -1)
    assert torch.allclose(rays_d, expect / expect.norm(dim=-1, keepdim=True), atol=1e-7)
    assert torch.allclose(rays_d.norm(dim=-1), torch.ones(2, 4), atol=1e-6)
    flat_o, flat_d = get_rays(dirs, c2w)
    assert flat_o.shape == (8, 3) and torch.equal(flat_d, rays_d.reshape(8, 3))
    both = torch.stack((c2w, torch.eye(4)))
    o2, d2 = get_rays(dirs, both, keepdim=True)
    assert o2.shape == (2, 2, 4, 3) and torch.equal(d2[0], rays_d) and torch.allclose(d2[1], dirs / dirs.norm(dim=-1, keepdim=True))
    o3, d3 = get_rays(dirs[None].expand(2, -1, -1, -1), both, keepdim=True)
    assert torch.equal(d3, d2) and torch.equal(o3, o2)
    o4, d4 = get_rays(dirs.reshape(-1, 3), c2w)
    assert torch.equal(d4, flat_d)
    o5, d5 = get_rays(dirs[0, :2], both)                             # one matrix per row
    assert torch.equal(d5[0], rays_d[0, 0]) and torch.equal(o5[1], torch.zeros(3))


# ---------------------------------------------------------------------------------------------------------------- the entry points
def test_entry_points_check_their_arguments_and_launch_nothing():
    from gaussianip_amd import _lib
    lib = _lib.model_lib()
    one, null = ctypes.c_void_p(256), ctypes.c_void_p(None)         # never dereferenced: every call below fails or has nothing to do
    box = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0, 4.0, 4.0, 4.0)

    def count(R=4, G=8, box=box, dt=0.01, near=0.0, far=1e10, K=64, ptrs=(one, one, one, null), counts=one):
        return lib.gip_volume_march_count(*ptrs, R, G, *box, dt, near, far, K, counts, null)

    def emit(R=4, G=8, box=box, dt=0.01, K=64, M=10, out=(one, one, one), offsets=one):
        return lib.gip_volume_march_emit(one, one, one, null, R, G, *box, dt, 0.0, 1e10, K, offsets, M, *out, null)
    for fn in (count, emit):
        assert fn(G=0) == 1 and fn(G=257) == 1 and fn(dt=0.0) == 1 and fn(dt=-1.0) == 1 and fn(dt=float("nan")) == 1 and fn(R=-1) == 1
        assert fn(K=0) == 1 and fn(R=1 << 21, K=1024) == 1 and fn(R=(1 << 31) // 64 + 1, K=1) == 1          # R K_cap >= 2^31
        assert fn(box=box[:3] + (-1.0,) + box[4:]) == 1 and fn(box=box[:6] + (0.0, 4.0, 4.0)) == 1 and fn(box=(float("nan"),) + box[1:]) == 1
        assert fn(R=0) == 0
    assert count(near=float("nan")) == 1 and count(ptrs=(null, one, one, null)) == 1 and count(ptrs=(one, one, null, null)) == 1
    assert count(counts=null) == 1
    assert emit(M=-1) == 1 and emit(M=1 << 31) == 1 and emit(out=(null, one, one)) == 1 and emit(offsets=null) == 1 and emit(M=0) == 0
    wf, wb = lib.gip_volume_weights_forward, lib.gip_volume_weights_backward
    assert wf(one, one, one, one, -1, 4, one, one, one, null) == 1 and wf(one, one, one, one, 4, -1, one, one, one, null) == 1
    assert wf(one, one, null, one, 4, 4, one, one, one, null) == 1 and wf(one, one, one, null, 4, 4, one, one, one, null) == 1
    assert wf(one, one, one, one, 4, 4, one, one, null, null) == 1
    assert wf(null, null, null, null, 0, 0, null, null, null, null) == 0 and wf(null, null, null, one, 4, 0, null, null, null, null) == 0
    assert wb(one, one, one, one, one, one, one, 4, 1 << 31, one, null) == 1 and wb(one, one, null, one, one, one, one, 4, 4, one, null) == 1
    assert wb(one, one, one, one, one, one, one, 4, 4, null, null) == 1 and wb(null, null, null, null, null, null, null, 0, 4, null, null) == 0
    af, ab = lib.gip_volume_accumulate_forward, lib.gip_volume_accumulate_backward
    assert af(one, one, one, 4, 4, 17, one, null) == 1 and af(one, one, one, 4, 4, 0, one, null) == 1 and af(one, null, one, 4, 4, 3, one, null) == 1
    assert af(one, one, null, 4, 4, 3, one, null) == 1 and af(one, one, one, 4, 4, 3, null, null) == 1 and af(null, one, one, 4, 4, 3, one, null) == 1
    assert af(one, one, one, 4, 1 << 28, 16, one, null) == 1 and af(null, null, null, 0, 0, 1, null, null) == 0
    assert ab(one, one, one, one, 4, 4, 17, one, one, null) == 1 and ab(one, null, one, one, 4, 4, 2, one, null, null) == 1
    assert ab(one, one, null, one, 4, 4, 3, one, one, null) == 1 and ab(one, one, one, one, 4, 4, 3, null, null, null) == 1
    assert ab(one, one, one, null, 4, 4, 3, one, one, null) == 1 and ab(null, null, null, null, 4, 0, 1, null, null, null) == 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_volume_kernels_do_not_spill(tmp_path):
    scratch, spilled, log = resource_usage("volume.hip", tmp_path / "o.o")
    for kernel in KERNELS:
        assert any(kernel in n for n in scratch), "no kernel-resource-usage remark for %s: %s" % (kernel, log[-500:])
    assert len(scratch) == len(KERNELS), sorted(scratch)
    bad = [(n, scratch[n], spilled.get(n, 0)) for n in scratch if scratch[n] or spilled.get(n, 0)]
    assert not bad, "kernels spilling: %s" % bad
