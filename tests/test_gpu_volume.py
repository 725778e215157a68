"""Volume rendering on the GPU (csrc/volume.hip, gaussianip_amd/utils/volume.py): the march, the compositing with its gradients, the
occupancy grid's pruning, the renderer over an implicit volume, a short fit, and GaussianModel.render_field_volume.

The march is compared bit for bit with the numpy float32 restatement of tests/volume_reference.py on the cases of tests/volume_inputs.py.
Everything else is compared with the float64 restatement under the rule of tests/test_gpu_hashgrid.py / test_gpu_isosurface.py: the
kernel's error over the quantity's maximum is at most 4 x the float32 op chain's own error on the same case (normalised the same way)
+ 1e-6.  Every element is compared.
With GIP_VOLUME_PARITY_OUT=<file> the figures are written there as JSON (profiles/volume_parity.json is such a run)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import field_inputs
import hashgrid_inputs
import volume_inputs as inputs
import volume_reference as reference

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 4.0, 1e-6
BG = (0.1, 0.2, 0.3)
_figures = {}


@pytest.fixture(scope="module", autouse=True)
def _write_figures():
    yield
    out = os.environ.get("GIP_VOLUME_PARITY_OUT")
    if out and _figures:
        with open(out, "w") as f:
            f.write(json.dumps(_figures, indent=1, sort_keys=True) + "\n")


def _cu(a):
    return torch.from_numpy(np.array(a)).cuda()                 # a copy: the cases' arrays are read-only


def _np(t):
    return t.detach().cpu().numpy()


def _counts():
    from gaussianip_amd import _lib
    return dict(_lib.call_counts)


def _launches(before):
    after = _counts()
    return {k: after[k] - before.get(k, 0) for k in after if after[k] != before.get(k, 0)}


def _rule(name, got, f64, chain):
    """The module's rule for one quantity: got (the kernels), f64 (the truth) and chain (the float32 op chain) as arrays."""
    got, f64, chain = (np.asarray(a, np.float64) for a in (got, f64, chain))
    assert got.shape == f64.shape == chain.shape and np.isfinite(got).all(), name
    mx = np.abs(f64).max()
    assert mx > 0, name
    err, ref_err = float(np.abs(got - f64).max() / mx), float(np.abs(chain - f64).max() / mx)
    bar = FACTOR * ref_err + FLOOR
    print("%s: kernel %.3e op chain %.3e bar %.3e (maximum %.3e)" % (name, err, ref_err, bar, mx))
    _figures[name] = dict(kernel_err=err, op_chain_err=ref_err, bar=bar, maximum=float(mx))
    assert err <= bar, (name, err, ref_err, bar)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _march(name):
    from gaussianip_amd.utils.volume import march_rays
    c = inputs.march_case(name)
    jitter = None if c["jitter"] is None else _cu(c["jitter"])
    return march_rays(_cu(c["rays_o"]), _cu(c["rays_d"]), _cu(c["occ"]), np.concatenate((c["lo"], c["hi"])), c["dt"], c["near"], c["far"], jitter,
                      c["K_cap"])


# ---------------------------------------------------------------------------------------------------------------- 1. the march is exact
@pytest.mark.parametrize("name", inputs.MARCH_CASES)
def test_the_march_is_exact(name):
    want = inputs.marched(name)
    R, M = inputs.march_case(name)["rays_o"].shape[0], want[0].shape[0]
    before = _counts()
    got = _march(name)
    # one count and one emit; without a sample nothing is emitted, without a ray nothing is counted either
    expected = {} if R == 0 else ({"gip_volume_march_count": 1} if M == 0 else {"gip_volume_march_count": 1, "gip_volume_march_emit": 1})
    assert _launches(before) == expected
    assert [t.dtype for t in got] == [torch.int32, torch.float32, torch.float32, torch.int32]
    for what, g, w in zip(("ray_indices", "t_starts", "t_ends", "offsets"), got, want):
        g = _np(g)
        assert g.shape == w.shape and np.array_equal(_bits(g), _bits(w)), (name, what, int((_bits(g) != _bits(w)).sum()) if g.shape == w.shape else g.shape)
    again = _march(name)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    print("%s: %d rays, %d samples, at most %d a ray" % (name, R, M, int(np.diff(want[3]).max()) if R else 0))


# ---------------------------------------------------------------------------------------------------------------- 2. weights and accumulate
@functools.lru_cache(maxsize=None)
def _composite_truth():
    """The compositing case's quantities twice: the float64 restatement, and the float32 op chain on the CPU.  Computed once and shared."""
    c = inputs.composite()
    f64, w_acc = reference.composite_f64(c)
    chained = reference.Chained(torch.float32)
    return f64, w_acc, reference.composite_run(c, w_acc, chained.render_weight_from_density, chained.accumulate_along_rays)


def _composite_kernels():
    from gaussianip_amd.utils import volume
    return reference.composite_run(inputs.composite(), _composite_truth()[1], volume.render_weight_from_density, volume.accumulate_along_rays,
                                   device="cuda")


def test_weights_and_accumulate():
    from gaussianip_amd.utils.volume import accumulate_along_rays, render_weight_from_density
    c = inputs.composite()
    f64, w_acc, chain = _composite_truth()
    before = _counts()
    got = _composite_kernels()
    n_acc = len(inputs.CHANNELS) + 1
    assert _launches(before) == {"gip_volume_weights_forward": 1, "gip_volume_weights_backward": 1, "gip_volume_accumulate_forward": n_acc,
                                 "gip_volume_accumulate_backward": n_acc}
    assert sorted(got) == sorted(f64)
    for name in sorted(f64):
        _rule("composite_%s" % name, got[name], f64[name], chain[name])
    again = _composite_kernels()
    for name in got:                                                 # forward and backward, bitwise
        assert np.array_equal(got[name].view(np.int64), again[name].view(np.int64)), name
    # rays without samples give exact zeros; the empty ray's transmittance never starts
    empty = np.flatnonzero(np.diff(c["offsets"]) == 0)
    assert empty.size >= 1
    for C in inputs.CHANNELS:
        assert not got["out_c%d" % C][empty].any()
    assert not got["out_none"][empty].any()
    # values=None equals values=ones
    w, idx, R = _cu(w_acc), _cu(c["ray_indices"]), c["n_rays"]
    assert torch.equal(accumulate_along_rays(w, None, idx, R), accumulate_along_rays(w, torch.ones((w.shape[0], 1), device="cuda"), idx, R))
    # one ray without ray_indices; int64 ray indices; a ray index outside [0, n_rays) contributes nothing, forward or backward
    a, b = int(c["offsets"][-2]), int(c["offsets"][-1])
    ts, te, sg = (_cu(c[k][a:b]) for k in ("t_starts", "t_ends", "sigmas"))
    whole = render_weight_from_density(_cu(c["t_starts"]), _cu(c["t_ends"]), _cu(c["sigmas"]), idx.long(), R)
    alone = render_weight_from_density(ts, te, sg)
    assert all(torch.equal(x[a:b], y) for x, y in zip(whole, alone))
    assert torch.equal(accumulate_along_rays(alone[0]), accumulate_along_rays(whole[0], None, idx, R)[-1:])
    wv = w.clone().requires_grad_(True)
    short = accumulate_along_rays(wv, None, idx, R - 1)
    (g_short,) = torch.autograd.grad(short.sum(), wv)
    assert torch.equal(short, accumulate_along_rays(w, None, idx, R)[:-1]) and not g_short[a:b].any() and (g_short[:a] == 1).all()
    # nothing to do: no samples, no rays
    none = torch.zeros(0, device="cuda")
    before = _counts()
    assert all(t.shape == (0,) for t in render_weight_from_density(none, none, none, torch.zeros(0, dtype=torch.int32, device="cuda"), 5))
    out = accumulate_along_rays(none, None, torch.zeros(0, dtype=torch.int32, device="cuda"), 5)
    assert out.shape == (5, 1) and not out.any() and _launches(before) == {}


# ---------------------------------------------------------------------------------------------------------------- 3. pruning
def _sample_keys(ray_indices, t_starts):
    return ray_indices.astype(np.int64) << 32 | _bits(t_starts).astype(np.int64) & 0xFFFFFFFF


def test_pruning_keeps_what_the_restatement_keeps():
    from gaussianip_amd.utils.volume import OccupancyGrid
    case, p = inputs.march_case("c_r257"), inputs.pruning()
    grid = OccupancyGrid(np.concatenate((case["lo"], case["hi"])), resolution=32).cuda()
    grid.binaries.copy_(_cu(case["occ"]).bool())
    sigmas = _cu(p["sigmas"])
    asked = []

    def sigma_fn(t_starts, t_ends, ray_indices):
        asked.append((t_starts, t_ends, ray_indices))
        return sigmas
    rays_o, rays_d = _cu(case["rays_o"]), _cu(case["rays_d"])
    kept = grid.sampling(rays_o, rays_d, sigma_fn=sigma_fn, render_step_size=case["dt"], alpha_thre=inputs.ALPHA_THRE,
                         early_stop_eps=inputs.EARLY_STOP_EPS)
    (seen,) = asked                                                  # the marched samples, exactly the restatement's
    assert all(np.array_equal(_bits(_np(a)), _bits(b)) for a, b in zip(seen, (p["t_starts"], p["t_ends"], p["ray_indices"])))
    _, trans, alphas = reference.weights_f64(p["t_starts"], p["t_ends"], p["sigmas"], p["offsets"])
    undecided = (np.abs(alphas - inputs.ALPHA_THRE) <= 1e-5) | (np.abs(trans - inputs.EARLY_STOP_EPS) <= 1e-4 * inputs.EARLY_STOP_EPS)
    want = (alphas >= inputs.ALPHA_THRE) & (trans >= inputs.EARLY_STOP_EPS)
    keys = _sample_keys(p["ray_indices"], p["t_starts"])
    assert np.unique(keys).size == keys.size
    got_keys = _sample_keys(_np(kept[0]), _np(kept[1]))
    got = np.isin(keys, got_keys)
    assert np.isin(got_keys, keys).all() and got.sum() == got_keys.size                 # a subset, nothing invented, order kept
    assert np.array_equal(got_keys, keys[got]) and np.array_equal(_bits(_np(kept[2])), _bits(p["t_ends"][got]))
    print("pruning: %d samples, %d kept, %d undecided, %d of them kept" % (keys.size, int(got.sum()), int(undecided.sum()), int((got & undecided).sum())))
    _figures["pruning"] = dict(samples=int(keys.size), kept=int(got.sum()), undecided=int(undecided.sum()))
    assert undecided.sum() <= 0.01 * keys.size
    assert np.array_equal(got[~undecided], want[~undecided])
    # without a sigma_fn, or with both thresholds at zero, nothing is pruned
    assert grid.sampling(rays_o, rays_d, render_step_size=case["dt"])[0].shape[0] == keys.size
    assert grid.sampling(rays_o, rays_d, sigma_fn=sigma_fn, render_step_size=case["dt"], early_stop_eps=0.0)[0].shape[0] == keys.size
    # stratified: a jitter in [0, 1) steps a ray, so every sample starts less than a step later than an unjittered one could
    torch.manual_seed(3)
    idx, ts, te = grid.sampling(rays_o, rays_d, render_step_size=case["dt"], stratified=True)
    assert idx.shape[0] > 0 and not np.array_equal(_bits(_np(ts[:64])), _bits(p["t_starts"][:64])) and bool((te > ts).all())


# ---------------------------------------------------------------------------------------------------------------- 4. argument checks
def test_argument_checks():
    import ctypes

    from gaussianip_amd import _lib
    from gaussianip_amd.utils.volume import accumulate_along_rays, march_rays, render_weight_from_density
    o, d = torch.rand(4, 3, device="cuda") - 2, torch.ones(4, 3, device="cuda")
    occ, box = torch.ones((8, 8, 8), dtype=torch.bool, device="cuda"), [-1, -1, -1, 1, 1, 1]
    before = _counts()
    for bad in ((o.double(), d), (o.cpu(), d.cpu()), (o, d.cpu()), (o[:, :2], d[:, :2]), (o, d[:3]), (o.reshape(-1), d.reshape(-1))):
        with pytest.raises(ValueError, match="float32 GPU"):
            march_rays(*bad, occ, box, 0.01)
    for bad_occ in (occ.cpu(), occ.float(), occ[:4], occ.reshape(-1), torch.ones((0, 0, 0), dtype=torch.bool, device="cuda"),
                    torch.ones((257, 257, 257), dtype=torch.bool, device="cuda")):
        with pytest.raises(ValueError, match="occ"):
            march_rays(o, d, bad_occ, box, 0.01)
    for dt in (0.0, -0.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="render_step_size"):
            march_rays(o, d, occ, box, dt)
    with pytest.raises(ValueError, match="aabb"):
        march_rays(o, d, occ, [-1, -1, -1, 1, -1, 1], 0.01)
    with pytest.raises(ValueError, match="jitter"):
        march_rays(o, d, occ, box, 0.01, jitter=torch.rand(3, device="cuda"))
    with pytest.raises(ValueError, match="31 bits"):                 # R K_cap >= 2^31
        march_rays(o, d, occ, box, 0.01, max_samples_per_ray=1 << 29)
    w, idx = torch.rand(6, device="cuda"), torch.tensor([0, 0, 1, 1, 1, 3], dtype=torch.int32, device="cuda")
    for bad in ((w.double(), w, w), (w.cpu(), w.cpu(), w.cpu()), (w, w, w[:5]), (w[:, None], w[:, None], w[:, None])):
        with pytest.raises(ValueError, match="float32 GPU"):
            render_weight_from_density(*bad, idx, 4)
    for bad_idx, n in ((idx.float(), 4), (idx.cpu(), 4), (idx[:5], 4), (idx, None), (idx, -1)):
        with pytest.raises(ValueError):
            render_weight_from_density(w, w, w, bad_idx, n)
    for bad_v in (torch.rand(6, 17, device="cuda"), torch.rand(6, 0, device="cuda"), torch.rand(5, 3, device="cuda"), torch.rand(6, device="cuda"),
                  torch.rand(6, 3), torch.rand(6, 3, device="cuda").double()):
        with pytest.raises(ValueError, match="values"):
            accumulate_along_rays(w, bad_v, idx, 4)
    with pytest.raises(ValueError, match="weights"):
        accumulate_along_rays(w.cpu(), None, idx.cpu(), 4)
    assert _launches(before) == {}
    # the entry points themselves: the bad-argument status, and nothing launched (the pointers are live, so a launch would be harmless)
    lib, null = _lib.model_lib(), ctypes.c_void_p(None)
    counts = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    unit = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0, 4.0, 4.0, 4.0)

    def count(R=4, G=8, dt=0.01, K=64):
        return lib.gip_volume_march_count(_lib.ptr(o), _lib.ptr(d), _lib.ptr(occ.view(torch.uint8)), null, R, G, *unit, dt, 0.0, 1e10, K,
                                          _lib.ptr(counts), null)
    assert count(G=0) == 1 and count(G=257) == 1 and count(dt=0.0) == 1 and count(dt=-1.0) == 1 and count(R=1 << 21, K=1024) == 1
    out = torch.full((4, 16), -7.0, device="cuda")
    offsets = torch.tensor([0, 2, 5, 5, 6], dtype=torch.int32, device="cuda")
    v = torch.rand(6, 16, device="cuda")
    assert lib.gip_volume_accumulate_forward(_lib.ptr(w), _lib.ptr(v), _lib.ptr(offsets), 4, 6, 17, _lib.ptr(out), null) == 1
    assert lib.gip_volume_accumulate_backward(_lib.ptr(w), _lib.ptr(v), _lib.ptr(idx), _lib.ptr(out), 4, 6, 17, _lib.ptr(w), _lib.ptr(v), null) == 1
    torch.cuda.synchronize()
    assert (counts == -7).all() and (out == -7).all()


# ---------------------------------------------------------------------------------------------------------------- 5. the renderer
def _look_at(position):
    """c2w [4, 4] of a camera at `position` looking at the origin: x right, y up, looking along -z."""
    p = np.asarray(position, np.float64)
    z = p / np.linalg.norm(p)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, np.cross(z, x), z, p
    return torch.from_numpy(c2w.astype(np.float32))


def _rays(size=16):
    """2 views of size x size rays around the origin from a distance of 3; the corners of each image miss the box [-1, 1]^3."""
    from gaussianip_amd.utils.volume import get_ray_directions, get_rays
    c2w = torch.stack((_look_at((0.0, 0.0, 3.0)), _look_at((2.0, 1.0, -2.0))))
    rays_o, rays_d = get_rays(get_ray_directions(size, size, 0.6 * size), c2w, keepdim=True)
    return rays_o.cuda().contiguous(), rays_d.cuda().contiguous()


def _misses(rays_o, rays_d, lo, hi):
    o, d = _np(rays_o).reshape(-1, 3), _np(rays_d).reshape(-1, 3)
    return np.array([reference.ray_span(o[r], d[r], np.asarray(lo, np.float32), np.asarray(hi, np.float32), 0.0, 1e10) is None for r in range(o.shape[0])])


def _volume(seed=31):
    from gaussianip_amd.utils.volume import ImplicitVolume
    torch.manual_seed(seed)
    volume = ImplicitVolume(radius=1.0, pos_encoding_config=dict(hashgrid_inputs.CONFIG_SMALL)).cuda()
    with torch.no_grad():
        volume.encoding.encoding.params.uniform_(-0.5, 0.5)          # features that vary over the blob
    return volume


class _patched:
    """utils.volume with render_weight_from_density and accumulate_along_rays replaced by the op chain in `dtype` (None: the kernels).
    The march and the occupancy grid's own pruning stay the kernels', so every variant composites the same samples."""

    def __init__(self, monkeypatch, dtype):
        self.monkeypatch, self.dtype = monkeypatch, dtype

    def __enter__(self):
        from gaussianip_amd.utils import volume
        self.context = self.monkeypatch.context()
        m = self.context.__enter__()
        if self.dtype is not None:
            chained = reference.Chained(self.dtype)
            m.setattr(volume, "render_weight_from_density", chained.render_weight_from_density)
            m.setattr(volume, "accumulate_along_rays", chained.accumulate_along_rays)

    def __exit__(self, *exc):
        return self.context.__exit__(*exc)


def test_the_renderer(monkeypatch):
    from gaussianip_amd.utils.volume import NeRFVolumeRenderer
    volume = _volume()
    renderer = NeRFVolumeRenderer(volume, num_samples_per_ray=64).cuda().eval()
    assert not renderer.estimator.binaries.any()                     # as nerfacc's: empty until update_step has seen the density
    rays_o, rays_d = _rays()
    bg = torch.tensor(BG, device="cuda")
    with torch.no_grad():
        blank = renderer(rays_o, rays_d, bg_color=bg)
    assert torch.equal(blank["comp_rgb"], bg.expand(2, 16, 16, 3)) and not blank["opacity"].any() and not blank["depth"].any()
    renderer.estimator.binaries.fill_(True)
    outs = {}
    for kind, dtype in (("kernel", None), ("float32", torch.float32), ("float64", torch.float64)):
        before = _counts()
        with _patched(monkeypatch, dtype), torch.no_grad():
            outs[kind] = renderer(rays_o, rays_d, bg_color=bg)
        used = _launches(before)
        # the sampling prunes with the kernels in every variant; the compositing uses them only in the first
        assert used["gip_volume_weights_forward"] == (2 if dtype is None else 1) and used.get("gip_volume_accumulate_forward", 0) == (4 if dtype is None else 0)
    out = outs["kernel"]
    assert sorted(out) == ["comp_rgb", "comp_rgb_bg", "comp_rgb_fg", "depth", "opacity", "z_variance"]
    assert tuple(out["comp_rgb"].shape) == (2, 16, 16, 3) and tuple(out["z_variance"].shape) == (2, 16, 16, 1) and out["comp_rgb"].dtype == torch.float32
    for name in ("comp_rgb", "comp_rgb_fg", "opacity", "depth", "z_variance"):
        _rule("renderer_%s" % name, _np(out[name]), _np(outs["float64"][name]), _np(outs["float32"][name]))
    miss = torch.from_numpy(_misses(rays_o, rays_d, [-1] * 3, [1] * 3)).cuda().view(2, 16, 16)
    assert 0 < int(miss.sum()) < miss.numel()
    assert torch.equal(out["comp_rgb"][miss], bg.expand(int(miss.sum()), 3)) and not out["opacity"][miss].any()
    assert float(out["opacity"].max()) > 0.9 and float(out["z_variance"].min()) >= 0
    # the other shapes of the background, and none
    with torch.no_grad():
        per_view = renderer(rays_o, rays_d, bg_color=bg.expand(2, 3))["comp_rgb"]
        per_pixel = renderer(rays_o, rays_d, bg_color=bg.expand(2, 16, 16, 3))["comp_rgb"]
        black = renderer(rays_o, rays_d)
    assert torch.equal(per_view, out["comp_rgb"]) and torch.equal(per_pixel, out["comp_rgb"])
    assert torch.equal(black["comp_rgb"], black["comp_rgb_fg"]) and torch.equal(black["comp_rgb_fg"], out["comp_rgb_fg"])
    with pytest.raises(ValueError):
        renderer(rays_o, rays_d, bg_color=torch.zeros(5, 3))
    with pytest.raises(ValueError):
        renderer(rays_o.reshape(-1, 3), rays_d.reshape(-1, 3))


# ---------------------------------------------------------------------------------------------------------------- 6. the loop closes
STEPS = 10
SAMPLES = 64


class _Blob(torch.nn.Module):
    """An analytic field over [-1, 1]^3: density 30 exp(-|p|^2 / (2 x 0.3^2)) and a smooth colour of the position, as features."""
    radius = 1.0

    def __init__(self):
        super().__init__()
        self.register_buffer("bbox", torch.tensor([[-1.0] * 3, [1.0] * 3]))

    def forward_density(self, points):
        return 30.0 * torch.exp(-(points ** 2).sum(-1, keepdim=True) / (2 * 0.3 ** 2))

    def forward(self, points, output_normal=False):
        colour = 0.5 + 0.4 * torch.sin(points * torch.tensor([9.0, 7.0, 5.0], device=points.device) + 0.3)
        return {"density": self.forward_density(points), "features": torch.log(colour / (1.0 - colour))}


def _fit(monkeypatch, dtype, rays, target):
    from gaussianip_amd.utils.volume import NeRFVolumeRenderer
    volume = _volume(seed=41)
    renderer = NeRFVolumeRenderer(volume, num_samples_per_ray=SAMPLES, randomized=False, grid_prune=False).cuda().train()
    optimizer = torch.optim.Adam(renderer.parameters(), lr=0.01)
    bg = torch.tensor(BG, device="cuda")
    losses, first = [], None
    with _patched(monkeypatch, dtype):
        for step in range(STEPS + 1):
            optimizer.zero_grad()
            out = renderer(*rays, bg_color=bg)
            loss = ((out["comp_rgb"] - target) ** 2).mean()
            losses.append(float(loss.detach()))
            if step == STEPS:
                break
            loss.backward()
            if step == 0:
                first = dict(out=out, grads={k: p.grad.clone() for k, p in renderer.named_parameters()})
            optimizer.step()
    return renderer, losses, first


def test_the_loop_closes(monkeypatch):
    """The implicit volume in training mode without jitter or pruning, 2 views of 16 x 16 rays, the target an analytic blob rendered
    through the same march and compositing, STEPS Adam steps on all parameters: the loss falls, and the same steps with the op chain in
    place of the kernels give the same losses under the module's rule (the chain in float64 is the truth).  Then the occupancy grid
    learns the fitted density, and the pruned render stays within the weight it dropped."""
    from gaussianip_amd.utils.volume import NeRFVolumeRenderer
    rays = _rays()
    bg = torch.tensor(BG, device="cuda")
    with torch.no_grad():
        target = NeRFVolumeRenderer(_Blob().cuda(), num_samples_per_ray=SAMPLES, randomized=False, grid_prune=False).cuda().eval()(*rays, bg_color=bg)["comp_rgb"]
    assert float(target.std()) > 0.05
    before = _counts()
    renderer, losses, first = _fit(monkeypatch, None, rays, target)
    used = _launches(before)
    assert used["gip_volume_march_emit"] == STEPS + 1 and used["gip_volume_weights_backward"] == STEPS
    # four accumulates a render; the loss reads the colour and the opacity, so two of them run backward
    assert used["gip_volume_accumulate_forward"] == 4 * (STEPS + 1) and used["gip_volume_accumulate_backward"] == 2 * STEPS
    out = first["out"]
    M = out["weights"].shape[0]
    for key, shape in (("weights", (M, 1)), ("t_points", (M, 1)), ("t_intervals", (M, 1)), ("t_dirs", (M, 3)), ("points", (M, 3)), ("ray_indices", (M,)),
                       ("density", (M, 1)), ("features", (M, 3)), ("comp_rgb", (2, 16, 16, 3)), ("z_variance", (2, 16, 16, 1))):
        assert tuple(out[key].shape) == shape, key
    assert M > 1000 and "comp_normal" not in out
    grads = first["grads"]
    assert sorted(grads) == ["geometry.density_network.layers.0.weight", "geometry.density_network.layers.2.weight",
                             "geometry.encoding.encoding.params", "geometry.feature_network.layers.0.weight",
                             "geometry.feature_network.layers.2.weight"]
    assert all(bool(torch.isfinite(g).all()) and bool(g.any()) for g in grads.values())
    print("losses", " ".join("%.6f" % v for v in losses))
    assert len(losses) == STEPS + 1 and losses[-1] < losses[0]
    _, chain32, _ = _fit(monkeypatch, torch.float32, rays, target)
    _, chain64, _ = _fit(monkeypatch, torch.float64, rays, target)
    _rule("loop_losses", losses, chain64, chain32)
    _figures["loop"] = dict(steps=STEPS, losses=losses, losses_op_chain_float32=chain32, losses_op_chain_float64=chain64)

    # the occupancy grid learns the fitted density: all cells during warm-up (256 steps), then a quarter and the occupied ones
    pruned = NeRFVolumeRenderer(renderer.geometry, num_samples_per_ray=SAMPLES, randomized=False, grid_prune=True).cuda().train()
    assert not pruned.estimator.binaries.any()
    pruned.eval().update_step(0)                                     # not in training: nothing happens
    assert not pruned.estimator.binaries.any()
    pruned.train()
    torch.manual_seed(5)
    with torch.no_grad():
        for step in range(0, 256 + 2 * 16 + 1):
            pruned.update_step(step)
    occupied = int(pruned.estimator.binaries.sum())
    print("occupancy: %d of %d cells" % (occupied, 32 ** 3))
    assert 0 < occupied < 32 ** 3
    with torch.no_grad():
        full, part = renderer(*rays, bg_color=bg), pruned(*rays, bg_color=bg)
    kept = np.isin(_sample_keys(_np(full["ray_indices"]).astype(np.int32), _np(full["t_points"][:, 0])),
                   _sample_keys(_np(part["ray_indices"]).astype(np.int32), _np(part["t_points"][:, 0])))
    assert 0 < part["weights"].shape[0] < M and kept.sum() == part["weights"].shape[0]            # fewer samples, all of them the unpruned run's
    # Compositing is the expectation of the colour at the first sample that absorbs the ray, or of the background.  With the same
    # draws for both renders the outcome differs only when the unpruned ray is absorbed at a dropped sample, which has the probability
    # of the dropped samples' unpruned weights; colours and background lie in [0, 1], so that sum bounds the difference per channel.
    # 1e-5 is the float32 rounding of sums of at most 65 terms of at most 1.
    dropped = torch.zeros(2 * 16 * 16, device="cuda").index_add_(0, full["ray_indices"][~torch.from_numpy(kept).cuda()],
                                                                 full["weights"][~torch.from_numpy(kept).cuda(), 0])
    diff = (part["comp_rgb"] - full["comp_rgb"]).abs().amax(-1).reshape(-1)
    print("pruned render: %d of %d samples, difference at most %.3e, dropped weight at most %.3e" % (
        part["weights"].shape[0], M, float(diff.max()), float(dropped.max())))
    _figures["pruned_render"] = dict(samples=int(part["weights"].shape[0]), samples_unpruned=int(M), occupied_cells=occupied,
                                     max_difference=float(diff.max()), max_dropped_weight=float(dropped.max()))
    assert bool((diff <= dropped + 1e-5).all())


def test_normals_and_an_empty_batch():
    from gaussianip_amd.utils.volume import ImplicitVolume, NeRFVolumeRenderer
    rays_o, rays_d = _rays(8)
    for normal_type in ("finite_difference", "finite_difference_laplacian", "pred"):
        torch.manual_seed(2)
        volume = ImplicitVolume(pos_encoding_config=dict(hashgrid_inputs.CONFIG_SMALL), normal_type=normal_type).cuda()
        renderer = NeRFVolumeRenderer(volume, num_samples_per_ray=32, grid_prune=False, return_comp_normal=True).cuda().eval()
        with torch.no_grad():
            out = renderer(rays_o, rays_d)
        n = out["comp_normal"]
        assert tuple(n.shape) == (2, 8, 8, 3) and bool(torch.isfinite(n).all()) and float(n.min()) >= 0 and float(n.max()) <= 1 + 1e-6
        if normal_type != "pred":
            # The blob's density falls outwards and is symmetric about the chord's middle: mirrored samples have the same alpha and
            # opposite normal components along the ray, and the nearer one the higher transmittance, so the sum faces the camera.
            solid = out["opacity"][..., 0] > 0.5
            facing = ((2 * n / out["opacity"].clamp_min(1e-6) - 1) * -rays_d).sum(-1)
            assert int(solid.sum()) >= 8 and float(facing[solid].min()) > 0
    # every ray misses: the background, and gradients that are zero, not missing
    volume = _volume()
    renderer = NeRFVolumeRenderer(volume, num_samples_per_ray=32, randomized=False, grid_prune=False).cuda().train()
    away = -rays_d
    before = _counts()
    out = renderer(rays_o, away, bg_color=torch.tensor(BG, device="cuda"))
    assert out["weights"].shape == (0, 1) and torch.equal(out["comp_rgb"], torch.tensor(BG, device="cuda").expand(2, 8, 8, 3))
    out["comp_rgb"].sum().backward()
    assert set(_launches(before)) == {"gip_volume_march_count"}
    grads = [p.grad for p in renderer.parameters()]
    assert all(g is not None and not g.any() for g in grads)


# ---------------------------------------------------------------------------------------------------------------- 7. from the Gaussians
def _model():
    from gaussianip_amd.scene import GaussianModel
    cl, R, nb = field_inputs.case("b")
    gm = GaussianModel(0)
    gm._xyz, gm._opacity = _cu(cl["xyz"]), _cu(cl["opacity"])
    gm._scaling, gm._rotation = _cu(cl["scaling"]), _cu(cl["rotation"])
    P = cl["xyz"].shape[0]
    gm._features_dc = _cu(np.random.default_rng(3).standard_normal((P, 1, 3)).astype(np.float32))
    gm._features_rest = torch.zeros((P, 0, 3), device="cuda")
    return gm, dict(resolution=R, num_blocks=nb)


def test_render_field_volume(monkeypatch):
    from gaussianip_amd.scene.cameras import Camera
    from gaussianip_amd.utils.volume import get_ray_directions, get_rays
    gm, field = _model()
    H = W = 32
    fovy = 0.9
    c2w = _look_at((1.0, 0.8, 2.2))
    camera = Camera(c2w.cuda(), fovy, H, W)
    outs = {}
    for kind, dtype in (("kernel", None), ("float32", torch.float32), ("float64", torch.float64)):
        before = _counts()
        with _patched(monkeypatch, dtype):
            outs[kind] = gm.render_field_volume(camera, num_samples_per_ray=64, density_scale=0.5, bg_color=BG, **field)
        used = _launches(before)
        assert used["gip_volume_march_count"] == 1 == used["gip_volume_march_emit"]
        assert used.get("gip_volume_weights_forward", 0) == (1 if dtype is None else 0) and used.get("gip_volume_accumulate_forward", 0) == (3 if dtype is None else 0)
    out = outs["kernel"]
    assert tuple(out["comp_rgb"].shape) == (3, H, W) and tuple(out["opacity"].shape) == (1, H, W) == tuple(out["depth"].shape)
    assert all(out[k].dtype == torch.float32 and not out[k].requires_grad for k in out)
    for name in ("comp_rgb", "opacity", "depth"):
        _rule("field_volume_%s" % name, _np(out[name]), _np(outs["float64"][name]), _np(outs["float32"][name]))
    assert float(out["opacity"].max()) > 0.1 and float(out["opacity"].min()) >= 0
    # the rays of the same camera, built from its c2w the way the reference builds them; a ray that misses the box grown by a twentieth
    # certainly misses the box
    focal = 0.5 * H / np.tan(0.5 * fovy)
    rays_o, rays_d = get_rays(get_ray_directions(H, W, float(focal)), c2w, keepdim=True)
    half = 1.05 / gm.scale
    centre = _np(gm.center)
    miss = torch.from_numpy(_misses(rays_o, rays_d, centre - half, centre + half)).view(H, W).cuda()
    assert 0 < int(miss.sum()) < H * W
    bg = torch.tensor(BG, device="cuda")
    assert torch.equal(out["comp_rgb"][:, miss], bg[:, None].expand(3, int(miss.sum()))) and not out["opacity"][0, miss].any()
    hit = out["opacity"][0] > 0
    assert bool(hit.any()) and not (hit & miss).any()
    # depth is the weighted distance: inside the box's span along the ray wherever something was hit
    distance = float(np.linalg.norm(_np(c2w[:3, 3]) - centre))
    mean_depth = (out["depth"][0][hit] / out["opacity"][0][hit])
    assert float(mean_depth.min()) > distance - 1.8 / gm.scale and float(mean_depth.max()) < distance + 1.8 / gm.scale
    # black without a background; a denser field is more opaque; bad arguments
    black = gm.render_field_volume(camera, num_samples_per_ray=64, density_scale=0.5, **field)
    assert not black["comp_rgb"][:, miss].any() and torch.equal(black["opacity"], out["opacity"])
    denser = gm.render_field_volume(camera, num_samples_per_ray=64, density_scale=2.0, **field)
    assert float(denser["opacity"].sum()) > float(out["opacity"].sum())
    with pytest.raises(TypeError):
        gm.render_field_volume(camera, colour=1)
    with pytest.raises(ValueError):
        gm.render_field_volume(camera, grid_resolution=0, **field)
