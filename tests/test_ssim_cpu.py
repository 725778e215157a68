"""gaussianip_amd.utils.loss on the CPU: the PyTorch statement of SSIM (the path CPU tensors, other dtypes and other windows take)
against the reference's own numbers (tests/golden/ssim*.npz, tools/make_golden.py group `ssim`), the argument checks, 3-D input,
l1_loss / l2_loss.

The bar is the GPU test's: the statement evaluated in float64 is the reference point; per case and per quantity (scalar, per-image
vector, gradient normalised by max|grad_f64|) the float32 result may be off by at most 4 times the REFERENCE's float32 error
against that same float64 evaluation, plus a floor of 2e-6 (2e-6 of max|grad| for the gradient).  That alone would accept anything
next to a wrong golden file, so the golden numbers themselves must sit within 2e-3 of the float64 evaluation: the moments are
11 x 11 float32 sums of values <= 1 (error <= a few 1e-7 absolute), E[x^2] - mu^2 cancels against C2 = 9e-4 in the denominator,
so a map value is off by <= ~1e-3 relative and the means by less."""
import numpy as np
import pytest
import torch

import ssim_inputs
from gaussianip_amd.utils import l1_loss, l2_loss, ssim
from gaussianip_amd.utils import loss as loss_mod

FACTOR, FLOOR, GOLDEN_SANITY = 4.0, 2e-6, 2e-3


@pytest.fixture(scope="module")
def golden():
    return ssim_inputs.load_golden()


def _eval(a, b, dtype):
    x = torch.from_numpy(a).to(dtype).requires_grad_(True)
    y = torch.from_numpy(b).to(dtype)
    val = ssim(x, y)
    grad, = torch.autograd.grad(val, x)
    with torch.no_grad():
        vec = ssim(x, y, size_average=False)
    return float(val.detach()), vec.double().numpy(), grad.double().numpy()


@pytest.mark.parametrize("kind,shape", ssim_inputs.CASES, ids=[ssim_inputs.case_key(k, s) for k, s in ssim_inputs.CASES])
def test_fallback_matches_reference_numbers(golden, kind, shape):
    a, b = ssim_inputs.images(kind, shape)
    key = ssim_inputs.case_key(kind, shape)
    s64, v64, g64 = _eval(a, b, torch.float64)
    s32, v32, g32 = _eval(a, b, torch.float32)
    gs, gv, gg = float(golden[key + "_scalar"]), golden[key + "_vector"].astype(np.float64), golden[key + "_grad"].astype(np.float64)
    assert gv.shape == (shape[0],) and gg.shape == tuple(shape)
    ref_s, ref_v = abs(gs - s64), np.abs(gv - v64).max()
    got_s, got_v = abs(s32 - s64), np.abs(v32 - v64).max()
    print("%s scalar %.3e (ref %.3e) vector %.3e (ref %.3e)" % (key, got_s, ref_s, got_v, ref_v))
    assert ref_s <= GOLDEN_SANITY and ref_v <= GOLDEN_SANITY
    assert got_s <= FACTOR * ref_s + FLOOR
    assert got_v <= FACTOR * ref_v + FLOOR
    assert np.isfinite(g32).all()
    if kind == "same":
        # the gradient vanishes at img2 == img1; what float32 leaves is rounding residue, compared with the `near` case below
        assert abs(s32 - 1.0) <= 1e-6
        a2, b2 = ssim_inputs.images("near", shape)
        near = np.abs(_eval(a2, b2, torch.float32)[2]).max()
        print("%s max|grad| %.3e of near's" % (key, np.abs(g32).max() / near))
        assert np.abs(g32).max() <= 1e-3 * near
        return
    scale = np.abs(g64).max()
    ref_g, got_g = np.abs(gg - g64).max() / scale, np.abs(g32 - g64).max() / scale
    print("%s grad %.3e (ref %.3e)" % (key, got_g, ref_g))
    assert ref_g <= GOLDEN_SANITY
    assert got_g <= FACTOR * ref_g + FLOOR


def test_value_errors():
    a = torch.rand(3, 16, 16)
    with pytest.raises(ValueError, match="N, C, H, W"):
        ssim(a, a.clone(), size_average=False)
    b = torch.rand(1, 3, 16, 16)
    with pytest.raises(ValueError, match="img1 only"):
        ssim(b, b.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        ssim(b, torch.rand(1, 3, 16, 15))
    with torch.no_grad():      # nothing is differentiated: a target that happens to require grad is harmless
        assert torch.isfinite(ssim(b, b.clone().requires_grad_(True)))


def test_three_dimensional_input_is_one_image():
    a, b = ssim_inputs.images("near", (1, 3, 11, 11))
    x4, y4 = torch.from_numpy(a), torch.from_numpy(b)
    v3, v4 = ssim(x4[0], y4[0]), ssim(x4, y4)
    assert v3.dim() == 0 and torch.equal(v3, v4)
    assert ssim(x4, y4, size_average=False).shape == (1,)


def test_other_windows_take_the_same_statement():
    """window_size != 11: a 7-tap window against the dense definition written out with unfold, float64."""
    a, b = ssim_inputs.images("rand", (1, 3, 11, 11))
    x, y = torch.from_numpy(a).double(), torch.from_numpy(b).double()
    w = loss_mod.gaussian_window(7).double().reshape(1, 49, 1)

    def blur(t):
        cols = torch.nn.functional.unfold(t.reshape(3, 1, 11, 11), 7, padding=3)      # [3, 49, 121]
        return (cols * w).sum(1).reshape(1, 3, 11, 11)
    mu1, mu2 = blur(x), blur(y)
    s1, s2, s12 = blur(x * x) - mu1 ** 2, blur(y * y) - mu2 ** 2, blur(x * y) - mu1 * mu2
    want = ((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4) / ((mu1 ** 2 + mu2 ** 2 + 1e-4) * (s1 + s2 + 9e-4))).mean()
    assert abs(float(ssim(x, y, window_size=7)) - float(want)) < 1e-12


def test_window_is_the_kernels_window():
    """The six distinct taps csrc/ssim.hip holds as hexadecimal literals are the float32 window of the PyTorch statement."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gaussianip_amd", "csrc", "ssim.hip")).read()
    taps = [float.fromhex(h) for h in re.findall(r"#define SSIM_W\d (0x[0-9a-f.]+p-?\d+)f", src)]
    w = loss_mod.gaussian_window(11)
    assert len(taps) == 6
    one_d = torch.tensor(taps + taps[-2::-1], dtype=torch.float32)
    assert torch.equal(torch.outer(one_d, one_d), w)


def test_l1_l2_closed_forms():
    a = torch.tensor([[0.0, 0.5], [1.0, 0.25]])
    b = torch.tensor([[0.5, 0.5], [0.0, 1.0]])
    assert float(l1_loss(a, b)) == pytest.approx((0.5 + 0.0 + 1.0 + 0.75) / 4)
    assert float(l2_loss(a, b)) == pytest.approx((0.25 + 0.0 + 1.0 + 0.5625) / 4)
    x = a.clone().requires_grad_(True)
    l2_loss(x, b).backward()
    assert torch.allclose(x.grad, 2 * (a - b) / 4)
