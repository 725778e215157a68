"""Image-space losses of the 3DGS trainers (gaussiansplatting/utils/loss_utils.py): l1_loss, l2_loss, ssim.

`ssim` on float32 CUDA images with the 11-tap window runs as one forward and one backward HIP kernel (csrc/ssim.hip,
include/gip_model.h: gip_ssim_*); everything else (CPU tensors, other dtypes, other window sizes) takes `ssim_torch`, a plain
PyTorch statement of the same definition — under GIP_STRICT=1 a CUDA tensor that would leave the kernels raises instead.
The photometric loss of those trainers is `0.8 * l1_loss(a, b) + 0.2 * (1 - ssim(a, b))`."""
import math
import os

import torch
import torch.nn.functional as F

C1 = 0.01 ** 2
C2 = 0.03 ** 2
fallback_counts = {}     # site -> CUDA calls that left the HIP kernels (whatever the GIP_STRICT level)


def l1_loss(network_output, gt):
    return (network_output - gt).abs().mean()


def l2_loss(network_output, gt):
    return (network_output - gt).square().mean()


def gaussian_window(window_size=11, sigma=1.5):
    """[window_size, window_size] float32: the taps exp(-(i - window_size // 2)^2 / (2 sigma^2)) rounded to float32, divided by their
    float32 sum, and the float32 outer product of that vector with itself."""
    half = window_size // 2
    taps = torch.tensor([math.exp(-((i - half) ** 2) / (2.0 * sigma * sigma)) for i in range(window_size)], dtype=torch.float32)
    taps = taps / taps.sum()
    return torch.outer(taps, taps)


def ssim_map_torch(img1, img2, window_size=11):
    """The SSIM map, same shape as the images ([N, C, H, W] or [C, H, W]), in the images' dtype: zero-padded depthwise window
    means of x, y, x^2, y^2, x y, then (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2))."""
    channels = img1.shape[-3]
    kernel = gaussian_window(window_size).to(device=img1.device, dtype=img1.dtype).expand(channels, 1, window_size, window_size).contiguous()

    def blur(t):
        return F.conv2d(t, kernel, padding=window_size // 2, groups=channels)

    mu1, mu2 = blur(img1), blur(img2)
    var1 = blur(img1 * img1) - mu1 * mu1
    var2 = blur(img2 * img2) - mu2 * mu2
    cov = blur(img1 * img2) - mu1 * mu2
    return ((2 * mu1 * mu2 + C1) * (2 * cov + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (var1 + var2 + C2))


def ssim_torch(img1, img2, window_size=11, size_average=True):
    """`ssim` as PyTorch ops (any device, any floating dtype, any odd window)."""
    m = ssim_map_torch(img1, img2, window_size)
    return m.mean() if size_average else m.mean(1).mean(1).mean(1)


def _left_the_kernels(site, t):
    fallback_counts[site] = fallback_counts.get(site, 0) + 1
    if int(os.environ.get("GIP_STRICT", "0") or 0) >= 1:
        raise RuntimeError("GIP_STRICT: %s left the HIP kernels for a PyTorch FALLBACK (tensor %s, %s)" % (site, tuple(t.shape), t.dtype))


class _FusedSSIM(torch.autograd.Function):
    """Per-image SSIM means [N] of [N, C, H, W] float32 CUDA images; optionally the map.  Saves the two images and the three
    derivative planes [3, N, C, H, W] the forward kernel wrote; the backward kernel reads the upstream gradient [N] on the device."""

    @staticmethod
    def forward(ctx, img1, img2, want_map):
        from .. import _lib
        N, C, H, W = img1.shape
        dev = img1.device
        need_grad = ctx.needs_input_grad[0]
        ws = torch.empty(max(1, _lib.model_lib().gip_ssim_workspace_bytes(N, C, H, W) // 4), dtype=torch.float32, device=dev)
        means = torch.empty(N, dtype=torch.float32, device=dev)
        deriv = torch.empty((3, N, C, H, W), dtype=torch.float32, device=dev) if need_grad else None
        smap = torch.empty_like(img1) if want_map else None
        _lib.call_model(dev, "gip_ssim_forward", _lib.ptr(img1), _lib.ptr(img2), N, C, H, W, _lib.ptr(means), _lib.ptr(deriv), _lib.ptr(smap),
                        _lib.ptr(ws))
        if need_grad:
            ctx.save_for_backward(img1, img2, deriv)
        if want_map:
            ctx.mark_non_differentiable(smap)
            return means, smap
        return means, None

    @staticmethod
    def backward(ctx, g_means, _g_map):
        from .. import _lib
        img1, img2, deriv = ctx.saved_tensors
        N, C, H, W = img1.shape
        g = g_means.to(torch.float32).contiguous()
        g_img1 = torch.empty_like(img1)
        _lib.call_model(img1.device, "gip_ssim_backward", _lib.ptr(img1), _lib.ptr(img2), _lib.ptr(deriv), _lib.ptr(g), N, C, H, W,
                        _lib.ptr(g_img1))
        return g_img1, None, None


def _fused_ok(img1, img2, window_size):
    return (img1.is_cuda and img2.is_cuda and img1.dtype == torch.float32 and img2.dtype == torch.float32 and window_size == 11
            and img1.numel() > 0)


def ssim_with_map(img1, img2):
    """(per-image means [N], SSIM map [N, C, H, W]) of 4-D float32 CUDA images from the fused kernel (diagnostics and tests; the map
    carries no gradient)."""
    _check(img1, img2, False)
    if not _fused_ok(img1, img2, 11):
        raise ValueError("ssim_with_map needs float32 CUDA images")
    means, smap = _FusedSSIM.apply(img1.contiguous(), img2.contiguous(), True)
    return means, smap


def _check(img1, img2, size_average):
    if img1.shape != img2.shape or img1.dim() not in (3, 4):
        raise ValueError("ssim needs two images of one shape, [N, C, H, W] or [C, H, W]; got %s and %s" % (tuple(img1.shape), tuple(img2.shape)))
    if img1.dim() == 3 and not size_average:
        raise ValueError("ssim(size_average=False) returns one value per image and needs [N, C, H, W] input; got %s" % (tuple(img1.shape),))
    if img2.requires_grad and torch.is_grad_enabled():
        raise ValueError("ssim differentiates with respect to img1 only: img2 is the target image and must not require grad "
                         "(detach it, or swap the arguments)")


def ssim(img1, img2, window_size=11, size_average=True):
    """loss_utils.py:33-63: the mean SSIM of two images (a scalar), or with size_average=False one mean per image [N]."""
    _check(img1, img2, size_average)
    if not _fused_ok(img1, img2, window_size):
        if img1.is_cuda:
            _left_the_kernels("ssim", img1)
        return ssim_torch(img1, img2, window_size, size_average)
    a, b = (img1, img2) if img1.dim() == 4 else (img1.unsqueeze(0), img2.unsqueeze(0))
    means, _ = _FusedSSIM.apply(a.contiguous(), b.contiguous(), False)
    return means.mean() if size_average else means
