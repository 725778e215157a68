"""NeuS volume rendering on the GPU (csrc/volume_sdf.hip, gaussianip_amd/utils/sdf_volume.py): the weights from alpha, the fused render
with its gradients, the occupancy grid's pruning by alpha, the renderer over an implicit SDF, a short fit, and the isosurface.

The rule is that of tests/test_gpu_volume.py, with its numbers: every element is compared, and the kernel's error over the quantity's
maximum is at most 4 x the float32 op chain's own error on the same case (normalised the same way) + 1e-6, both errors taken against
the float64 restatement (tests/sdf_volume_reference.py; for the renderer and the fit, the same ops in float64 on the GPU).
With GIP_SDF_VOLUME_PARITY_OUT=<file> the figures are written there as JSON (profiles/sdf_volume_parity.json is such a run)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import hashgrid_inputs
import sdf_volume_inputs as inputs
import sdf_volume_reference as reference
import volume_inputs
import volume_reference

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 4.0, 1e-6
BG = (0.1, 0.2, 0.3)
_figures = {}


@pytest.fixture(scope="module", autouse=True)
def _write_figures():
    yield
    out = os.environ.get("GIP_SDF_VOLUME_PARITY_OUT")
    if out and _figures:
        with open(out, "w") as f:
            f.write(json.dumps(_figures, indent=1, sort_keys=True) + "\n")


def _cu(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()          # a copy: the cases' arrays are read-only


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


def _same_bits(a, b):
    return all(np.array_equal(a[k].view(np.int64), b[k].view(np.int64)) for k in a)


# ---------------------------------------------------------------------------------------------------------------- 1. weights from alpha
@functools.lru_cache(maxsize=None)
def _case_alphas():
    """The case's alphas at beta = 300 (53 of them exactly 1), rounded once to float32."""
    c = inputs.composite()
    return reference.render_f64(c, 300.0, 1.0, c["normals"], None)["alphas"].astype(np.float32)


def _weights_kernels(alphas, c):
    from gaussianip_amd.utils.sdf_volume import render_weight_from_alpha
    a = _cu(alphas).requires_grad_(True)
    weights, trans = render_weight_from_alpha(a, _cu(c["ray_indices"]), c["n_rays"])
    assert not trans.requires_grad
    (g,) = torch.autograd.grad((weights * _cu(c["g_weights"])).sum(), a)
    return {k: _np(v).astype(np.float64) for k, v in dict(weights=weights, trans=trans, g_alphas=g).items()}


def test_render_weight_from_alpha():
    from gaussianip_amd.utils.sdf_volume import render_weight_from_alpha
    c, alphas = inputs.composite(), _case_alphas()
    assert (alphas == 1.0).sum() >= 10
    w, trans = reference.weights_from_alpha_f64(alphas, c["offsets"])
    f64 = dict(weights=w, trans=trans, g_alphas=reference.weights_from_alpha_backward_f64(alphas, c["offsets"], c["g_weights"]))
    chain = reference.weights_chain(alphas, c["offsets"], c["g_weights"])
    before = _counts()
    got = _weights_kernels(alphas, c)
    assert _launches(before) == {"gip_volume_alpha_weights_forward": 1, "gip_volume_alpha_weights_backward": 1}
    for name in sorted(f64):
        _rule("alpha_weights_%s" % name, got[name], f64[name], chain[name])
    assert all(np.isfinite(v).all() for v in got.values())            # at alpha == 1 too, where the division form is 0 / 0
    assert _same_bits(got, _weights_kernels(alphas, c))
    # behind a sample with alpha == 1 nothing is seen
    lo = int(c["offsets"][8])
    assert not got["weights"][lo + 151:lo + 200].any() and not got["trans"][lo + 151:lo + 200].any()
    # one ray without ray_indices; int64 indices; nothing to do
    a, b = int(c["offsets"][9]), int(c["offsets"][10])
    idx = _cu(c["ray_indices"])
    whole = render_weight_from_alpha(_cu(alphas), idx.long(), c["n_rays"])
    alone = render_weight_from_alpha(_cu(alphas[a:b]))
    assert all(torch.equal(x[a:b], y) for x, y in zip(whole, alone))
    none = torch.zeros(0, device="cuda")
    before = _counts()
    assert all(t.shape == (0,) for t in render_weight_from_alpha(none, torch.zeros(0, dtype=torch.int32, device="cuda"), 5))
    assert _launches(before) == {}
    for bad in (_cu(alphas).double(), _cu(alphas).cpu(), _cu(alphas)[:, None]):
        with pytest.raises(ValueError, match="float32 GPU"):
            render_weight_from_alpha(bad, idx.to(bad.device), c["n_rays"])


# ---------------------------------------------------------------------------------------------------------------- 2. the fused render
@functools.lru_cache(maxsize=None)
def _truth(beta, rho, with_normals, C):
    c = inputs.composite()
    args = (beta, rho) + reference.variant_arrays(c, with_normals, C) + (c["g_weights"],)
    return reference.render_all_f64(c, *args), reference.render_chain(c, *args)


def _leaves(c, beta, with_normals, C):
    normals, values, g_out = reference.variant_arrays(c, with_normals, C)
    sdf = _cu(c["sdf"]).requires_grad_(True)
    n = None if normals is None else _cu(normals).requires_grad_(True)
    v = None if values is None else _cu(values).requires_grad_(True)
    inv_std = torch.tensor([beta], device="cuda", requires_grad=True)
    return sdf, n, v, inv_std, _cu(g_out)


def _finish(c, leaves, out, weights, alphas, trans=None):
    sdf, n, v, inv_std, g_out = leaves
    named = [(k, x) for k, x in (("g_sdf", sdf), ("g_normals", n), ("g_values", v), ("g_inv_std", inv_std)) if x is not None]
    grads = torch.autograd.grad((out * g_out).sum() + (weights * _cu(c["g_weights"])).sum(), [x for _, x in named])
    res = dict(alphas=alphas, weights=weights, out=out, **{k: g for (k, _), g in zip(named, grads)})
    if trans is not None:
        res["trans"] = trans
    return {k: _np(t).astype(np.float64) for k, t in res.items()}


def _fused(beta, rho, with_normals, C):
    from gaussianip_amd.utils.sdf_volume import render_sdf_rays
    c = inputs.composite()
    leaves = _leaves(c, beta, with_normals, C)
    out, weights, alphas = render_sdf_rays(leaves[0], leaves[1], _cu(c["rays_d"]), _cu(c["t_starts"]), _cu(c["t_ends"]), leaves[2], leaves[3],
                                           _cu(c["ray_indices"]), c["n_rays"], rho)
    assert not alphas.requires_grad and tuple(out.shape) == (c["n_rays"], 2 + C)
    return _finish(c, leaves, out, weights, alphas)


def _fused_forward_buffers(beta, rho, with_normals, C):
    """gip_volume_sdf_render_forward on buffers of the test's own: its four outputs, trans among them, which render_sdf_rays keeps for
    its backward and does not return."""
    from gaussianip_amd._lib import call_model, ptr
    c = inputs.composite()
    normals, values, _ = reference.variant_arrays(c, with_normals, C)
    sdf, n, d, ts, te, v, offsets = [_cu(a) for a in (c["sdf"], normals, c["rays_d"], c["t_starts"], c["t_ends"], values, c["offsets"])]
    inv_std = torch.tensor([beta], device="cuda")
    R, M = c["n_rays"], sdf.shape[0]
    alphas, trans, weights = (torch.full((M,), float("nan"), device="cuda") for _ in range(3))
    out = torch.zeros((R, 2 + C), device="cuda")
    call_model(sdf.device, "gip_volume_sdf_render_forward", ptr(sdf), ptr(n), ptr(d), ptr(ts), ptr(te), ptr(v), ptr(offsets), ptr(inv_std), rho,
               R, M, C, ptr(alphas), ptr(trans), ptr(weights), ptr(out))
    return {k: _np(t).astype(np.float64) for k, t in dict(alphas=alphas, trans=trans, weights=weights, out=out).items()}


def _primitives(beta, rho, with_normals, C):
    """The three-primitive path on the GPU: neus_alpha, render_weight_from_alpha, accumulate_along_rays."""
    from gaussianip_amd.utils.sdf_volume import neus_alpha, render_weight_from_alpha
    from gaussianip_amd.utils.volume import accumulate_along_rays
    c = inputs.composite()
    leaves = _leaves(c, beta, with_normals, C)
    idx, R, ts, te = _cu(c["ray_indices"]), c["n_rays"], _cu(c["t_starts"]), _cu(c["t_ends"])
    alphas = neus_alpha(leaves[0], leaves[1], _cu(c["rays_d"])[idx.long()], te - ts, leaves[3], rho)
    weights, trans = render_weight_from_alpha(alphas.contiguous(), idx, R)
    parts = [accumulate_along_rays(weights, None, idx, R), accumulate_along_rays(weights, ((ts + te) * 0.5)[:, None].contiguous(), idx, R)]
    if leaves[2] is not None:
        parts.append(accumulate_along_rays(weights, leaves[2], idx, R))
    return _finish(c, leaves, torch.cat(parts, dim=1), weights, alphas, trans)


@pytest.mark.parametrize("beta,rho,with_normals,C", inputs.variants())
def test_render_sdf_rays(beta, rho, with_normals, C):
    c = inputs.composite()
    f64, chain = _truth(beta, rho, with_normals, C)
    before = _counts()
    got = _fused(beta, rho, with_normals, C)
    assert _launches(before) == {"gip_volume_sdf_render_forward": 1, "gip_volume_sdf_render_backward": 1}
    tag = "sdf_render_b%g_r%g_%s_c%d" % (beta, rho, "n" if with_normals else "nonormals", C)
    # render_sdf_rays returns no trans: the kernel's own comes from the entry point on the test's buffers, with the same bits elsewhere
    buffers = _fused_forward_buffers(beta, rho, with_normals, C)
    assert _same_bits({k: buffers[k] for k in ("alphas", "weights", "out")}, got)
    got["trans"] = buffers["trans"]
    assert sorted(got) == sorted(f64)
    for name in sorted(got):
        _rule("%s_%s" % (tag, name), got[name], f64[name], chain[name])
    del got["trans"]
    assert _same_bits(got, _fused(beta, rho, with_normals, C))       # forward and backward, bitwise
    empty = np.flatnonzero(np.diff(c["offsets"]) == 0)
    assert empty.size == 2 and not got["out"][empty].any()
    if beta == 300.0:
        assert (got["alphas"] == 1.0).sum() >= 10


@pytest.mark.parametrize("beta,with_normals,C", [(300.0, True, 3), (20.0, True, 16), (300.0, False, 0)])
def test_the_fused_render_agrees_with_the_three_primitives(beta, with_normals, C):
    f64, chain = _truth(beta, 0.3, with_normals, C)
    before = _counts()
    parts = _primitives(beta, 0.3, with_normals, C)
    used = _launches(before)
    assert used["gip_volume_alpha_weights_forward"] == 1 and used["gip_volume_accumulate_forward"] == (3 if C else 2)
    fused = _fused(beta, 0.3, with_normals, C)
    fused["trans"] = _fused_forward_buffers(beta, 0.3, with_normals, C)["trans"]
    for name in sorted(parts):
        _rule("primitives_b%g_c%d_%s" % (beta, C, name), parts[name], f64[name], chain[name])
        # the two paths against each other: the fused error may be at most the rule's multiple of the primitives' own
        _rule("fused_vs_primitives_b%g_c%d_%s" % (beta, C, name), fused[name], f64[name], parts[name])


def test_render_sdf_rays_arguments():
    from gaussianip_amd.utils.sdf_volume import render_sdf_rays
    c = inputs.composite()
    sdf, n, d, ts, te, v = [_cu(a) for a in (c["sdf"], c["normals"], c["rays_d"], c["t_starts"], c["t_ends"], c["values"][3])]
    beta, idx, R = torch.tensor([20.0], device="cuda"), _cu(c["ray_indices"]), c["n_rays"]
    before = _counts()
    for bad in ((sdf.double(), n, d, ts, te, v, beta, idx, R), (sdf.cpu(), n, d, ts, te, v, beta, idx, R), (sdf, n[:5], d, ts, te, v, beta, idx, R),
                (sdf, n, d[:5], ts, te, v, beta, idx, R), (sdf, n, d, ts[:5], te, v, beta, idx, R), (sdf, n, d, ts, te, v[:, :0], beta, idx, R),
                (sdf, n, d, ts, te, torch.zeros((1005, 17), device="cuda"), beta, idx, R), (sdf, n, d, ts, te, v, 20.0, idx, R),
                (sdf, n, d, ts, te, v, beta.cpu(), idx, R), (sdf, n, d, ts, te, v, beta, None, None), (sdf, n, d, ts, te, v, beta, idx, R, 1.5),
                (sdf, n, d, ts, te, v, beta, idx, R, float("nan"))):
        with pytest.raises(ValueError):
            render_sdf_rays(*bad)
    # no samples: zeros, nothing launched, and zero gradients
    none = torch.zeros(0, device="cuda", requires_grad=True)
    b = beta.clone().requires_grad_(True)
    out, weights, alphas = render_sdf_rays(none, None, d, none.detach(), none.detach(), None, b, torch.zeros(0, dtype=torch.int32, device="cuda"), R)
    assert tuple(out.shape) == (R, 2) and not out.any() and weights.shape == (0,)
    out.sum().backward()
    assert _launches(before) == {} and float(b.grad) == 0.0


# ---------------------------------------------------------------------------------------------------------------- 3. pruning
def _sample_keys(ray_indices, t_starts):
    return ray_indices.astype(np.int64) << 32 | np.ascontiguousarray(t_starts).view(np.int32).astype(np.int64) & 0xFFFFFFFF


def test_pruning_by_alpha_keeps_what_the_restatement_keeps():
    from gaussianip_amd.utils.volume import OccupancyGrid
    case, p = volume_inputs.march_case("c_r257"), inputs.pruning()
    grid = OccupancyGrid(np.concatenate((case["lo"], case["hi"])), resolution=32).cuda()
    grid.binaries.copy_(_cu(case["occ"]).bool())
    alphas = _cu(p["alphas"])
    asked = []

    def alpha_fn(t_starts, t_ends, ray_indices):
        asked.append(t_starts)
        return alphas
    rays_o, rays_d = _cu(case["rays_o"]), _cu(case["rays_d"])
    before = _counts()
    kept = grid.sampling(rays_o, rays_d, alpha_fn=alpha_fn, render_step_size=case["dt"], alpha_thre=inputs.ALPHA_THRE,
                         early_stop_eps=inputs.EARLY_STOP_EPS)
    used = _launches(before)
    assert used.get("gip_volume_alpha_weights_forward") == 1 and "gip_volume_weights_forward" not in used
    assert len(asked) == 1 and np.array_equal(_np(asked[0]).view(np.int32), p["t_starts"].view(np.int32))
    _, trans = reference.weights_from_alpha_f64(p["alphas"], p["offsets"])
    a64 = p["alphas"].astype(np.float64)
    undecided = (np.abs(a64 - inputs.ALPHA_THRE) <= 1e-5) | (np.abs(trans - inputs.EARLY_STOP_EPS) <= 1e-4 * inputs.EARLY_STOP_EPS)
    want = (a64 >= inputs.ALPHA_THRE) & (trans >= inputs.EARLY_STOP_EPS)
    keys = _sample_keys(p["ray_indices"], p["t_starts"])
    got_keys = _sample_keys(_np(kept[0]), _np(kept[1]))
    got = np.isin(keys, got_keys)
    assert np.isin(got_keys, keys).all() and got.sum() == got_keys.size and np.array_equal(got_keys, keys[got])
    print("pruning: %d samples, %d kept, %d undecided" % (keys.size, int(got.sum()), int(undecided.sum())))
    _figures["pruning"] = dict(samples=int(keys.size), kept=int(got.sum()), undecided=int(undecided.sum()))
    assert undecided.sum() <= 0.01 * keys.size
    assert np.array_equal(got[~undecided], want[~undecided])
    assert grid.sampling(rays_o, rays_d, alpha_fn=alpha_fn, render_step_size=case["dt"], early_stop_eps=0.0)[0].shape[0] == keys.size
    with pytest.raises(ValueError, match="not both"):
        grid.sampling(rays_o, rays_d, sigma_fn=alpha_fn, alpha_fn=alpha_fn, render_step_size=case["dt"])


# ---------------------------------------------------------------------------------------------------------------- 4. the renderer
def _chain_render(dtype):
    """render_sdf_rays as a chain of torch ops in `dtype` on the samples' device: neus_alpha, the exclusive cumprod of 1 - alpha along
    every ray (the rays laid out as the rows of a dense matrix padded with ones) and index_add_."""
    from gaussianip_amd.utils.sdf_volume import neus_alpha

    def render(sdf, normals, rays_d, t_starts, t_ends, values, inv_std, ray_indices, n_rays, cos_anneal_ratio=1.0):
        idx, M = ray_indices.long(), sdf.shape[0]
        ts, te = t_starts.to(dtype), t_ends.to(dtype)
        alphas = neus_alpha(sdf.to(dtype), None if normals is None else normals.to(dtype), rays_d.to(dtype)[idx], te - ts, inv_std.to(dtype),
                            cos_anneal_ratio)
        cols = [torch.ones((M, 1), dtype=dtype, device=sdf.device), ((ts + te) / 2)[:, None]] + ([] if values is None else [values.to(dtype)])
        width = sum(col.shape[1] for col in cols)
        if M == 0:
            return torch.zeros((n_rays, width), dtype=dtype, device=sdf.device) + 0 * inv_std.to(dtype).sum(), alphas, alphas.detach()
        first = torch.searchsorted(idx, torch.arange(n_rays, device=idx.device))
        pos = torch.arange(M, device=idx.device) - first[idx]
        dense = torch.ones((n_rays, int(pos.max()) + 2), dtype=dtype, device=sdf.device).index_put((idx, pos + 1), 1 - alphas)
        trans = torch.cumprod(dense, dim=1)[idx, pos]
        weights = trans * alphas
        out = torch.zeros((n_rays, width), dtype=dtype, device=sdf.device).index_add_(0, idx, weights[:, None] * torch.cat(cols, dim=1))
        return out, weights, alphas.detach()
    return render


class _patched:
    """utils.sdf_volume with render_sdf_rays replaced by the op chain in `dtype` (None: the kernel).  The march and the occupancy grid's
    own pruning stay the kernels', so every variant composites the same samples."""

    def __init__(self, monkeypatch, dtype):
        self.monkeypatch, self.dtype = monkeypatch, dtype

    def __enter__(self):
        from gaussianip_amd.utils import sdf_volume
        self.context = self.monkeypatch.context()
        m = self.context.__enter__()
        if self.dtype is not None:
            m.setattr(sdf_volume, "render_sdf_rays", _chain_render(self.dtype))

    def __exit__(self, *exc):
        return self.context.__exit__(*exc)


def _look_at(position):
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


def _geometry(seed=31, **kwargs):
    from gaussianip_amd.utils.sdf_volume import ImplicitSDF
    torch.manual_seed(seed)
    geometry = ImplicitSDF(radius=1.0, pos_encoding_config=dict(hashgrid_inputs.CONFIG_SMALL), sdf_bias="sphere", sdf_bias_params=0.5, **kwargs).cuda()
    with torch.no_grad():
        geometry.encoding.encoding.params.uniform_(-0.1, 0.1)        # features that vary over the sphere, which the bias still shapes
    return geometry


def test_the_renderer(monkeypatch):
    from gaussianip_amd.utils.sdf_volume import NeuSVolumeRenderer
    geometry = _geometry()
    fused = NeuSVolumeRenderer(geometry, num_samples_per_ray=64).cuda().eval()
    unfused = NeuSVolumeRenderer(geometry, num_samples_per_ray=64, fused=False).cuda().eval()
    assert not fused.estimator.binaries.any()                        # as nerfacc's: empty until update_step has seen the field
    rays_o, rays_d = _rays()
    bg = torch.tensor(BG, device="cuda")
    with torch.no_grad():
        blank = fused(rays_o, rays_d, bg_color=bg)
    assert torch.equal(blank["comp_rgb"], bg.expand(2, 16, 16, 3)) and not blank["opacity"].any()
    for r in (fused, unfused):
        r.estimator.binaries.fill_(True)
    outs = {}
    for kind, renderer, dtype in (("fused", fused, None), ("unfused", unfused, None), ("float32", fused, torch.float32), ("float64", fused, torch.float64)):
        before = _counts()
        with _patched(monkeypatch, dtype), torch.no_grad():
            outs[kind] = renderer(rays_o, rays_d, bg_color=bg)
        used = _launches(before)
        # the sampling prunes with the primitive in every variant; one fused launch, or the primitive again and four accumulates
        assert used.get("gip_volume_sdf_render_forward", 0) == (1 if kind == "fused" else 0), kind
        assert used["gip_volume_alpha_weights_forward"] == (2 if kind == "unfused" else 1) and used.get("gip_volume_accumulate_forward", 0) == (4 if kind == "unfused" else 0)
    out = outs["fused"]
    assert sorted(out) == ["comp_normal", "comp_rgb", "comp_rgb_bg", "comp_rgb_fg", "depth", "inv_std", "opacity"]
    assert tuple(out["comp_rgb"].shape) == (2, 16, 16, 3) == tuple(out["comp_normal"].shape) and out["comp_rgb"].dtype == torch.float32
    assert float(out["inv_std"]) == pytest.approx(np.exp(3.0), rel=1e-5)
    for name in ("comp_rgb", "comp_rgb_fg", "opacity", "depth", "comp_normal"):
        _rule("renderer_fused_%s" % name, _np(out[name]), _np(outs["float64"][name]), _np(outs["float32"][name]))
        _rule("renderer_unfused_%s" % name, _np(outs["unfused"][name]), _np(outs["float64"][name]), _np(outs["float32"][name]))
    o, d = _np(rays_o).reshape(-1, 3), _np(rays_d).reshape(-1, 3)
    lo, hi = np.full(3, -1, np.float32), np.full(3, 1, np.float32)
    miss = torch.from_numpy(np.array([volume_reference.ray_span(o[r], d[r], lo, hi, 0.0, 1e10) is None for r in range(o.shape[0])])).cuda().view(2, 16, 16)
    assert 0 < int(miss.sum()) < miss.numel()
    for kind in ("fused", "unfused"):
        assert torch.equal(outs[kind]["comp_rgb"][miss], bg.expand(int(miss.sum()), 3)) and not outs[kind]["opacity"][miss].any()
    assert float(out["opacity"].max()) > 0.9
    # the sphere's normals face the camera where it is solid
    solid = out["opacity"][..., 0] > 0.9
    facing = ((2 * out["comp_normal"] / out["opacity"].clamp_min(1e-6) - 1) * -rays_d).sum(-1)
    assert int(solid.sum()) >= 8 and float(facing[solid].median()) > 0
    volsdf = NeuSVolumeRenderer(geometry, num_samples_per_ray=64, use_volsdf=True).cuda().eval()
    volsdf.estimator.binaries.fill_(True)
    before = _counts()
    with torch.no_grad():
        vol = volsdf(rays_o, rays_d, bg_color=bg)
    assert "gip_volume_sdf_render_forward" not in _launches(before)
    assert all(bool(torch.isfinite(vol[k]).all()) for k in vol) and float(vol["opacity"].max()) > 0.5
    with pytest.raises(ValueError):
        fused(rays_o.reshape(-1, 3), rays_d.reshape(-1, 3))
    with pytest.raises(ValueError):
        fused(rays_o, rays_d, bg_color=torch.zeros(5, 3))


# ---------------------------------------------------------------------------------------------------------------- 5. the loop closes
STEPS = 10
SAMPLES = 64


class _Sphere(torch.nn.Module):
    """An analytic sphere of radius 0.6 in [-1, 1]^3 with a smooth colour of the position, as features."""
    radius = 1.0

    def __init__(self):
        super().__init__()
        self.register_buffer("bbox", torch.tensor([[-1.0] * 3, [1.0] * 3]))

    def forward_sdf(self, points):
        return points.norm(dim=-1, keepdim=True) - 0.6

    def forward(self, points, output_normal=False):
        colour = 0.5 + 0.4 * torch.sin(points * torch.tensor([9.0, 7.0, 5.0], device=points.device) + 0.3)
        normal = torch.nn.functional.normalize(points, dim=-1)
        return {"sdf": self.forward_sdf(points), "features": torch.log(colour / (1.0 - colour)), "normal": normal}


def _fit(monkeypatch, dtype, fused, rays, target):
    from gaussianip_amd.utils.sdf_volume import NeuSVolumeRenderer
    geometry = _geometry(seed=41)
    renderer = NeuSVolumeRenderer(geometry, num_samples_per_ray=SAMPLES, randomized=False, grid_prune=False, fused=fused).cuda().train()
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
    return losses, first


def test_the_loop_closes(monkeypatch):
    """The implicit SDF in training mode without jitter or pruning, 2 views of 16 x 16 rays, the target an analytic sphere of radius
    0.6 rendered through the same call, STEPS Adam steps on all parameters: the loss falls with the fused call and with the three
    primitives, and both give the losses of the float64 op chain under the module's rule."""
    from gaussianip_amd.utils.sdf_volume import NeuSVolumeRenderer
    rays = _rays()
    bg = torch.tensor(BG, device="cuda")
    with torch.no_grad():
        target = NeuSVolumeRenderer(_Sphere().cuda(), num_samples_per_ray=SAMPLES, randomized=False, grid_prune=False).cuda().eval()(*rays, bg_color=bg)["comp_rgb"]
    assert float(target.std()) > 0.05
    before = _counts()
    losses, first = _fit(monkeypatch, None, True, rays, target)
    used = _launches(before)
    assert used["gip_volume_sdf_render_forward"] == STEPS + 1 and used["gip_volume_sdf_render_backward"] == STEPS
    assert "gip_volume_alpha_weights_forward" not in used and "gip_volume_accumulate_forward" not in used
    out = first["out"]
    M = out["weights"].shape[0]
    for key, shape in (("weights", (M, 1)), ("t_points", (M, 1)), ("t_intervals", (M, 1)), ("t_dirs", (M, 3)), ("points", (M, 3)), ("ray_indices", (M,)),
                       ("sdf", (M, 1)), ("features", (M, 3)), ("normal", (M, 3)), ("sdf_grad", (M, 3)), ("comp_rgb", (2, 16, 16, 3)), ("inv_std", ())):
        assert tuple(out[key].shape) == shape, key
    assert M > 1000 and "comp_normal" not in out
    grads = first["grads"]
    assert sorted(grads) == ["geometry.encoding.encoding.params", "geometry.feature_network.layers.0.weight", "geometry.feature_network.layers.2.weight",
                             "geometry.sdf_network.layers.0.weight", "geometry.sdf_network.layers.2.weight", "variance._inv_std"]
    assert all(bool(torch.isfinite(g).all()) and bool(g.any()) for g in grads.values())
    before = _counts()
    losses_unfused, first_unfused = _fit(monkeypatch, None, False, rays, target)
    used = _launches(before)
    assert "gip_volume_sdf_render_forward" not in used and used["gip_volume_alpha_weights_backward"] == STEPS
    assert all(bool(g.any()) for g in first_unfused["grads"].values())
    print("losses fused  ", " ".join("%.6f" % v for v in losses))
    print("losses unfused", " ".join("%.6f" % v for v in losses_unfused))
    assert len(losses) == STEPS + 1 == len(losses_unfused) and losses[-1] < losses[0] and losses_unfused[-1] < losses_unfused[0]
    chain32, _ = _fit(monkeypatch, torch.float32, True, rays, target)
    chain64, _ = _fit(monkeypatch, torch.float64, True, rays, target)
    _rule("loop_losses_fused", losses, chain64, chain32)
    _rule("loop_losses_unfused", losses_unfused, chain64, chain32)
    _figures["loop"] = dict(steps=STEPS, losses_fused=losses, losses_unfused=losses_unfused, losses_op_chain_float32=chain32,
                            losses_op_chain_float64=chain64)


def test_update_step_and_an_empty_batch():
    from gaussianip_amd.utils.sdf_volume import NeuSVolumeRenderer
    rays_o, rays_d = _rays(8)
    geometry = _geometry()
    renderer = NeuSVolumeRenderer(geometry, num_samples_per_ray=32, randomized=False, cos_anneal_end_steps=100).cuda().train()
    torch.manual_seed(5)
    with torch.no_grad():
        renderer.update_step(0)
    assert renderer.cos_anneal_ratio == 0.0
    occupied = int(renderer.estimator.binaries.sum())
    assert 0 < occupied < 32 ** 3                                    # the shell around the sphere of radius 0.5
    renderer.update_step(50)
    assert renderer.cos_anneal_ratio == 0.5
    out = renderer(rays_o, rays_d)
    assert out["weights"].shape[0] > 0 and float(out["opacity"].detach().max()) > 0.5
    renderer.update_step(1000)
    assert renderer.cos_anneal_ratio == 1.0
    # every ray misses: the background, and gradients that are zero, not missing
    for fused in (True, False):
        renderer = NeuSVolumeRenderer(_geometry(), num_samples_per_ray=32, randomized=False, grid_prune=False, fused=fused).cuda().train()
        before = _counts()
        out = renderer(rays_o, -rays_d, bg_color=torch.tensor(BG, device="cuda"))
        assert out["weights"].shape == (0, 1) and torch.equal(out["comp_rgb"], torch.tensor(BG, device="cuda").expand(2, 8, 8, 3))
        out["comp_rgb"].sum().backward()
        assert set(_launches(before)) == {"gip_volume_march_count"}
        grads = [p.grad for p in renderer.parameters()]
        assert all(g is not None and not g.any() for g in grads), fused


# ---------------------------------------------------------------------------------------------------------------- 6. the isosurface
def _closed(faces):
    edges = np.sort(np.concatenate((faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]])), axis=1)
    _, counts = np.unique(edges, axis=0, return_counts=True)
    return bool((counts == 2).all())


def test_isosurface_hands_over_to_the_tet_stage():
    from gaussianip_amd.utils.sdf_volume import ImplicitSDF
    torch.manual_seed(3)
    geometry = ImplicitSDF(pos_encoding_config=dict(hashgrid_inputs.CONFIG_SMALL), sdf_bias="sphere", sdf_bias_params=0.5).cuda()
    resolution = 16
    with torch.no_grad():
        mesh = geometry.isosurface(resolution=resolution)
    v, f = _np(mesh.v_pos), _np(mesh.t_pos_idx)
    assert v.shape[0] > 100 and f.shape[0] > 200 and f.min() >= 0 and f.max() < v.shape[0]
    assert _closed(f)
    cell = 2.0 / resolution
    assert np.abs(np.linalg.norm(v, axis=1) - 0.5).max() <= cell
    # a shortened initialize_shape moves the field towards its shape; the surface is still closed
    fitted = ImplicitSDF(pos_encoding_config=dict(hashgrid_inputs.CONFIG_SMALL), shape_init="sphere", shape_init_params=0.5).cuda()
    points = torch.rand((2000, 3), device="cuda") * 2 - 1
    truth = points.norm(dim=-1, keepdim=True) - 0.5
    with torch.no_grad():
        before = float(((fitted.forward_sdf(points) - truth) ** 2).mean())
    fitted.initialize_shape(steps=30, batch=4000, lr=1e-2)
    with torch.no_grad():
        after = float(((fitted.forward_sdf(points) - truth) ** 2).mean())
    assert after < before
    # the vertices carry gradients to the field's parameters
    mesh = geometry.isosurface(resolution=resolution)
    mesh.v_pos.square().sum().backward()
    assert bool(geometry.sdf_network.layers[0].weight.grad.any())
