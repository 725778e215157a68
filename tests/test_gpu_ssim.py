"""The fused SSIM kernels (csrc/ssim.hip, gaussianip_amd.utils.loss.ssim) on the GPU.

Reference point: `_dense64`, the definition evaluated densely in float64 on the CPU with the 121-tap 2-D window (the float32
window of loss_utils.py:23-31 widened to float64) and differentiated by autograd.  Bar, per case and per quantity (map, per-image
means, scalar, gradient normalised by max|grad_f64|): the kernel's error against float64 is at most 4 times the REFERENCE's own
float32 error against float64 — from tests/golden/ssim*.npz (tools/make_golden.py group `ssim`: scalar, vector, gradient, and the
map's error figure) — plus a floor of 2e-6 (2e-6 of max|grad| for the gradient).  The kernel's tile is 32 x 32, so the six fixture
shapes are the issue's.  `same` (img2 == img1): the map is 1 within 1e-6, the gradient is finite and at most 1e-3 of the `near`
case's maximum at the same shape.

With GIP_SSIM_PARITY_OUT=<file> the per-case figures are written there as JSON (profiles/ssim_parity.json is such a run)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import scenes
import ssim_inputs

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 4.0, 2e-6
_figures = {}


@pytest.fixture(scope="module")
def golden():
    yield ssim_inputs.load_golden()
    out = os.environ.get("GIP_SSIM_PARITY_OUT")
    if out and _figures:
        with open(out, "w") as f:
            json.dump(_figures, f, indent=1, sort_keys=True)


def _window64():
    taps = np.array([np.exp(-((i - 5) ** 2) / 4.5) for i in range(11)]).astype(np.float32)
    taps = taps / torch.from_numpy(taps).sum().numpy()            # float32 sum in torch's order, like the reference's
    return torch.from_numpy(np.outer(taps, taps).astype(np.float32)).double()


@functools.lru_cache(maxsize=None)
def _dense64(kind, shape, upstream=None):
    """(map, per-image means, scalar, d (sum_n upstream[n] * mean_n) / d img1) in float64; upstream None = the scalar's gradient."""
    a, b = ssim_inputs.images(kind, shape)
    x = torch.from_numpy(a).double().requires_grad_(True)
    y = torch.from_numpy(b).double()
    C = shape[1]
    w = _window64().expand(C, 1, 11, 11).contiguous()

    def blur(t):
        return torch.nn.functional.conv2d(t, w, padding=5, groups=C)
    mu1, mu2 = blur(x), blur(y)
    s1, s2, s12 = blur(x * x) - mu1 * mu1, blur(y * y) - mu2 * mu2, blur(x * y) - mu1 * mu2
    m = (2 * mu1 * mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2) / ((mu1 * mu1 + mu2 * mu2 + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    means = m.mean(dim=(1, 2, 3))
    target = means.mean() if upstream is None else (means * torch.tensor(upstream, dtype=torch.float64)).sum()
    grad, = torch.autograd.grad(target, x)
    return m.detach().numpy(), means.detach().numpy(), float(means.mean().detach()), grad.numpy()


def _gpu(kind, shape):
    a, b = ssim_inputs.images(kind, shape)
    return torch.from_numpy(a).cuda().requires_grad_(True), torch.from_numpy(b).cuda()


def _kernel(kind, shape):
    """map, means, scalar, gradient of the scalar from the kernel path, as float64 numpy."""
    from gaussianip_amd.utils import loss
    x, y = _gpu(kind, shape)
    means_m, smap = loss.ssim_with_map(x.detach(), y)
    val = loss.ssim(x, y)
    grad, = torch.autograd.grad(val, x)
    with torch.no_grad():
        vec = loss.ssim(x, y, size_average=False)
    assert torch.equal(vec, means_m)
    return smap.double().cpu().numpy(), vec.double().cpu().numpy(), float(val.detach()), grad.double().cpu().numpy()


def _check(key, name, err, ref_err):
    bar = FACTOR * ref_err + FLOOR
    _figures.setdefault(key, {})[name] = {"kernel_err": err, "reference_err": ref_err, "ratio": (err / ref_err) if ref_err > 0 else None,
                                          "bar": bar}
    print("%s %s: kernel %.3e reference %.3e bar %.3e" % (key, name, err, ref_err, bar))
    assert err <= bar, (key, name, err, ref_err)


def _compare(golden, kind, shape, with_golden_grad=True):
    from gaussianip_amd import _lib
    before = dict(_lib.call_counts)
    key = ssim_inputs.case_key(kind, shape)
    m64, v64, s64, g64 = _dense64(kind, shape)
    smap, vec, val, grad = _kernel(kind, shape)
    assert _lib.call_counts.get("gip_ssim_forward", 0) > before.get("gip_ssim_forward", 0)
    assert _lib.call_counts.get("gip_ssim_backward", 0) > before.get("gip_ssim_backward", 0)
    assert np.isfinite(smap).all() and np.isfinite(grad).all()
    _check(key, "map", np.abs(smap - m64).max(), float(golden[key + "_map_err"]))
    _check(key, "means", np.abs(vec - v64).max(), np.abs(golden[key + "_vector"].astype(np.float64) - v64).max())
    _check(key, "scalar", abs(val - s64), abs(float(golden[key + "_scalar"]) - s64))
    if kind == "same":
        assert np.abs(smap - 1.0).max() <= 1e-6
        near = np.abs(_kernel("near", shape)[3]).max()
        _figures[key]["grad_max_over_near"] = float(np.abs(grad).max() / near)
        assert np.abs(grad).max() <= 1e-3 * near
        return
    scale = np.abs(g64).max()
    ref_g = (np.abs(golden[key + "_grad"].astype(np.float64) - g64).max() / scale) if with_golden_grad else float(golden[key + "_grad_err"])
    _check(key, "grad", np.abs(grad - g64).max() / scale, ref_g)


@pytest.mark.parametrize("kind,shape", ssim_inputs.CASES, ids=[ssim_inputs.case_key(k, s) for k, s in ssim_inputs.CASES])
def test_kernel_path_against_float64(golden, kind, shape):
    _compare(golden, kind, shape)


def test_stage_three_shape(golden):
    """(4, 3, 415, 290), render-like images: 13 x 10 tiles per plane, partial in both directions."""
    _compare(golden, *ssim_inputs.STAGE3_CASE, with_golden_grad=False)


def test_bitwise_repeatable():
    from gaussianip_amd.utils import loss
    runs = []
    for _ in range(2):
        x, y = _gpu("rand", (2, 3, 45, 67))
        vec = loss.ssim(x, y, size_average=False)
        grad, = torch.autograd.grad(vec.sum(), x)
        runs.append((vec.detach().clone(), grad.clone(), loss.ssim_with_map(x.detach(), y)[1]))
    for p, q in zip(*runs):
        assert torch.equal(p, q)


def test_forward_only_path_is_bitwise_the_training_forward():
    from gaussianip_amd.utils import loss
    for shape in ((2, 3, 45, 67), (1, 1, 33, 65)):
        x, y = _gpu("smooth", shape)
        train = loss.ssim(x, y)
        train_vec = loss.ssim(x, y, size_average=False)
        assert train.requires_grad
        with torch.no_grad():
            plain, plain_vec = loss.ssim(x, y), loss.ssim(x, y, size_average=False)
        assert not plain.requires_grad and torch.equal(plain, train.detach()) and torch.equal(plain_vec, train_vec.detach())
        assert torch.equal(loss.ssim(x.detach(), y), train.detach())
        assert torch.equal(loss.ssim(x.detach()[0], y[0]), loss.ssim(x.detach()[:1], y[:1]))      # [C, H, W] = one image


def test_upstream_gradients(golden):
    from gaussianip_amd.utils import loss
    kind, shape = "near", (2, 3, 45, 67)
    key = ssim_inputs.case_key(kind, shape)
    # the gradient of image n is linear in the upstream gradient of ITS mean alone, and the scalar is the mean of the N means:
    # under an upstream vector `up` the reference's float32 gradient (and its error) of image n is the golden one times N up[n]
    _, _, _, g_scalar = _dense64(kind, shape)
    ref_err = np.abs(golden[key + "_grad"].astype(np.float64) - g_scalar)
    ref = ref_err.max() / np.abs(g_scalar).max()
    up = (0.25, -1.5)
    x, y = _gpu(kind, shape)
    vec = loss.ssim(x, y, size_average=False)
    grad, = torch.autograd.grad((vec * torch.tensor(up, device="cuda")).sum(), x)
    g64 = _dense64(kind, shape, up)[3]
    ref_up = max(abs(u) * shape[0] * ref_err[n].max() for n, u in enumerate(up)) / np.abs(g64).max()
    _check(key + "_upstream", "grad_vector", np.abs(grad.double().cpu().numpy() - g64).max() / np.abs(g64).max(), ref_up)
    x, y = _gpu(kind, shape)
    grad, = torch.autograd.grad(0.2 * (1.0 - loss.ssim(x, y)), x)
    g64 = -0.2 * g_scalar
    _check(key + "_upstream", "grad_scaled_scalar", np.abs(grad.double().cpu().numpy() - g64).max() / np.abs(g64).max(), ref)


def test_strict_mode(monkeypatch):
    from gaussianip_amd.utils import loss
    x, y = _gpu("rand", (1, 3, 11, 11))
    monkeypatch.setenv("GIP_STRICT", "1")
    with pytest.raises(RuntimeError, match="GIP_STRICT"):
        loss.ssim(x, y, window_size=7)
    with pytest.raises(RuntimeError, match="GIP_STRICT"):
        loss.ssim(x.double(), y.double())
    assert torch.isfinite(loss.ssim(x, y, window_size=11))
    monkeypatch.setenv("GIP_STRICT", "0")
    assert torch.isfinite(loss.ssim(x, y, window_size=7))
    with pytest.raises(ValueError, match="img1 only"):
        loss.ssim(x, y.clone().requires_grad_(True))


def test_stage_three_step_with_ssim_term():
    """StageThreeStep(lambda_ssim=0.2) on the scene of test_gpu_pipeline.test_stage_three_step_with_lpips_term (the smallest stage-3
    scene of the suite): loss = the lambda_ssim = 0 loss + 0.2 (1 - ssim(small, gt)), the term evaluated by the PyTorch statement
    on the same `small`; every Gaussian parameter gets a finite gradient; lambda_ssim = 0.0 is bitwise the step without the
    argument."""
    import math
    from argparse import ArgumentParser
    import torch.nn.functional as F
    from gaussianip_amd.arguments import OptimizationParams, PipelineParams
    from gaussianip_amd.scene import Camera, GaussianModel
    from gaussianip_amd.system import StageThreeStep
    from gaussianip_amd.utils import BasicPointCloud
    from gaussianip_amd.utils.loss import ssim_torch
    rng = np.random.default_rng(6)
    P = 20000
    pts = scenes.human_points(P, rng).astype(np.float32)
    gm = GaussianModel(0)
    gm.create_from_pcd(BasicPointCloud(pts, np.full((P, 3), 0.5, np.float32), None), 4.0)
    gm.training_setup(OptimizationParams(ArgumentParser()))
    pipe = PipelineParams(ArgumentParser())
    bg = torch.ones(3, device="cuda")
    cams = [Camera(c2w=scenes.orbit_c2w(17.0, -180.0 + 90.0 * i, 1.5).cuda(), FoVy=math.radians(70.0), height=1024, width=1024)
            for i in range(4)]
    refined = torch.rand(4, 1024, 1024, 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    order, ids = [2, 0, 3, 1], [1, 3]
    without = StageThreeStep(gm, pipe, bg, cams, refined, order, train_bs=2).training_step(id_list=ids)
    zero = StageThreeStep(gm, pipe, bg, cams, refined, order, train_bs=2, lambda_ssim=0.0).training_step(id_list=ids)
    assert torch.equal(without["loss"], zero["loss"])
    st3 = StageThreeStep(gm, pipe, bg, cams, refined, order, train_bs=2, lambda_ssim=0.2)
    out = st3.training_step(id_list=ids)
    with torch.no_grad():
        img = out["render_pkg"]["render"][:, :, st3.CROP[0], st3.CROP[1]]
        small = F.interpolate(img, scale_factor=0.5, mode="bilinear", align_corners=False)
        gt = st3.gt_small[torch.as_tensor(ids, device="cuda")]
        assert small.shape == (2, 3, 415, 290)
        want = float(without["loss"]) + 0.2 * (1.0 - float(ssim_torch(small, gt)))
    got = float(out["loss"].detach())
    assert abs(got - want) <= 1e-5 * abs(want), (got, want)
    gm.optimizer.zero_grad(set_to_none=True)
    out["loss"].backward()
    for grp in gm.optimizer.param_groups:
        gr = grp["params"][0].grad
        assert gr is not None and torch.isfinite(gr).all(), grp["name"]
    assert float(gm._features_dc.grad.abs().max()) > 0
