"""NeuS volume rendering without a GPU (csrc/volume_sdf.hip, gaussianip_amd/utils/sdf_volume.py): the exported symbols, what the
compositing case promises, the float64 restatement's hand-written gradients against torch float64 autograd and against central
differences on a case with alpha == 1 samples, the textbook division form shown to be non-finite there, the float32 op chain against
the restatement, the PyTorch formulas and modules on CPU tensors, the entry points' argument checks (which launch nothing), the share
of undecided samples in the GPU pruning test's inputs and the compiler's resource report of every kernel of the file."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import sdf_volume_inputs as inputs
import sdf_volume_reference as reference
from test_model_no_spills_cpu import HIPCC, resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("volume_alpha_weights_forward_kernel", "volume_alpha_weights_backward_kernel", "volume_sdf_render_forward_kernel",
           "volume_sdf_render_backward_kernel")
SYMBOLS = ["gip_volume_alpha_weights_forward", "gip_volume_alpha_weights_backward", "gip_volume_sdf_render_forward",
           "gip_volume_sdf_render_backward"]
SMALL_GRID = {"otype": "HashGrid", "n_levels": 2, "n_features_per_level": 2, "log2_hashmap_size": 6, "base_resolution": 4, "per_level_scale": 1.5}


def test_symbols_exported():
    from gaussianip_amd import _lib
    from gaussianip_amd.utils import sdf_volume
    so = os.path.join(ROOT, "gaussianip_amd", "lib", "libgip_model.so")
    assert os.path.exists(so), "libgip_model.so is not built"
    names = {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout.splitlines()
             if ln.strip()}
    lib = _lib.model_lib()
    with open(os.path.join(ROOT, "include", "gip_model.h")) as fh:
        header = fh.read()
    assert _lib.VOLUME_SDF_SYMBOLS == SYMBOLS
    for sym in SYMBOLS:
        assert sym in names and getattr(lib, sym) is not None and "int %s(" % sym in header, sym
    assert "neus_volume_renderer.py" in header
    with open(os.path.join(ROOT, "gaussianip_amd", "csrc", "Makefile")) as fh:
        assert fh.read().count("volume_sdf.hip") == 2                # a prerequisite of libgip_model.so and a source of its command
    assert sdf_volume.__all__ == ["render_weight_from_alpha", "neus_alpha", "volsdf_density", "render_sdf_rays", "LearnedVariance", "ImplicitSDF",
                                  "NeuSVolumeRenderer"]


# ---------------------------------------------------------------------------------------------------------------- the case
def _chain_alphas(beta, rho):
    from gaussianip_amd.utils.sdf_volume import neus_alpha
    c = inputs.composite()
    t = {k: torch.from_numpy(np.array(c[k])) for k in ("sdf", "normals", "rays_d", "t_starts", "t_ends")}
    dirs = t["rays_d"][torch.from_numpy(np.array(c["ray_indices"])).long()]
    return neus_alpha(t["sdf"], t["normals"], dirs, t["t_ends"] - t["t_starts"], torch.tensor(beta), rho).numpy()


def test_the_case_has_what_it_names():
    c = inputs.composite()
    counts = np.diff(c["offsets"])
    assert tuple(counts) == inputs.RAY_COUNTS and c["sdf"].shape == (1005,) and c["n_rays"] == 11 and c["n_rays"] % 4
    delta = c["t_ends"] - c["t_starts"]
    assert delta.dtype == np.float32 and (delta > 0).all() and (delta <= 0.01).all()
    forced = np.array([c["offsets"][r] + k for r, k in inputs.FORCED])
    assert (c["sdf"][forced] == -0.5).all() and len(forced) == 53
    free = np.setdiff1d(np.arange(1005), forced)
    assert c["sdf"][free].max() <= 0.1 and c["sdf"][free].min() >= -0.05
    cos = (c["rays_d"][c["ray_indices"]].astype(np.float64) * c["normals"]).sum(1)
    assert np.abs(cos).min() >= inputs.MIN_COS and 0.2 < (cos > 0).mean() < 0.4
    assert np.abs(np.linalg.norm(c["normals"].astype(np.float64), axis=1) - 1).max() < 1e-6
    for rho in inputs.RHOS:
        ones = _chain_alphas(300.0, rho) == 1.0
        print("rho %.1f: %d samples with alpha == 1 at beta 300" % (rho, int(ones.sum())))
        assert ones.sum() >= 10 and ones[forced].all()
        assert not (_chain_alphas(20.0, rho) == 1.0).any()
    assert len(inputs.variants()) == 32


# ---------------------------------------------------------------------------------------------------------------- gradients
def _variant(beta, rho, with_normals, C):
    c = inputs.composite()
    normals, values, g_out = reference.variant_arrays(c, with_normals, C)
    return c, (beta, rho, normals, values, g_out, c["g_weights"])


@pytest.mark.parametrize("beta,rho,with_normals,C", [(300.0, 0.3, True, 3), (300.0, 1.0, False, 0), (20.0, 1.0, True, 16), (20.0, 0.3, False, 1)])
def test_hand_written_backward_equals_autograd(beta, rho, with_normals, C):
    c, args = _variant(beta, rho, with_normals, C)
    mine, auto = reference.render_all_f64(c, *args), reference.render_autograd(c, *args)
    assert sorted(mine) == sorted(auto)
    for name in sorted(mine):
        mx = np.abs(auto[name]).max()
        assert mine[name].shape == auto[name].shape and np.isfinite(mine[name]).all() and mx > 0, name
        assert np.abs(mine[name] - auto[name]).max() <= 1e-10 * mx, (name, np.abs(mine[name] - auto[name]).max() / mx)
    if beta == 300.0:
        assert (mine["alphas"] == 1.0).sum() >= 10                   # exactly 1 in float64 too


def test_hand_written_backward_equals_central_differences():
    """beta = 300, where the forced samples have alpha == 1: the loss sum(out g_out) + sum(weights g_weights) differentiated by central
    differences in the sdf of the forced samples and of every seventh other one, in a normal and a value of each of those, and in beta."""
    c, args = _variant(300.0, 0.3, True, 3)
    beta, rho, normals, values, g_out, g_weights = args
    grads = reference.render_backward_f64(c, *args)

    def loss(sdf=c["sdf"], normals=normals, values=values, beta=beta):
        f = reference.render_f64(dict(c, sdf=sdf), beta, rho, normals, values)
        return (f["out"] * g_out).sum() + (f["weights"] * g_weights).sum()
    forced = [int(c["offsets"][r] + k) for r, k in inputs.FORCED]
    picked = sorted(set(forced[:6]) | set(range(0, 1005, 7)))
    assert (reference.render_f64(c, beta, rho, normals, values)["alphas"][forced] == 1.0).all()
    for name, array, h in (("g_sdf", c["sdf"], 1e-7), ("g_normals", normals, 1e-6), ("g_values", values, 1e-6)):
        x = np.array(array, np.float64)
        got, want = [], []
        for i in picked:
            at = (i,) if x.ndim == 1 else (i, i % x.shape[1])
            keep = x[at]
            x[at] = keep + h
            up = loss(**{name[2:]: x})
            x[at] = keep - h
            down = loss(**{name[2:]: x})
            x[at] = keep
            got.append(grads[name][at])
            want.append((up - down) / (2 * h))
        got, want = np.array(got), np.array(want)
        assert np.abs(got - want).max() <= 1e-5 * np.abs(grads[name]).max(), (name, np.abs(got - want).max(), np.abs(grads[name]).max())
    numeric = (loss(beta=beta + 1e-4) - loss(beta=beta - 1e-4)) / 2e-4
    assert abs(grads["g_inv_std"][0] - numeric) <= 1e-5 * abs(numeric)


def test_the_division_form_is_not_finite_at_alpha_one():
    c = inputs.composite()
    alphas = reference.render_f64(c, 300.0, 1.0, c["normals"], None)["alphas"]
    assert (alphas == 1.0).sum() >= 10
    divided = reference.weights_from_alpha_backward_division(alphas, c["offsets"], c["g_weights"])
    assert not np.isfinite(divided[alphas == 1.0]).any()
    recurrence = reference.weights_from_alpha_backward_f64(alphas, c["offsets"], c["g_weights"])
    auto = reference.weights_chain(alphas, c["offsets"], c["g_weights"], torch.float64)["g_alphas"]
    assert np.isfinite(recurrence).all() and np.abs(recurrence - auto).max() <= 1e-14 * np.abs(auto).max()
    fine = np.isfinite(divided)
    assert fine.sum() > 500 and np.abs(divided[fine] - recurrence[fine]).max() <= 1e-9 * np.abs(recurrence).max()


def test_op_chain_against_the_restatement():
    """float32 against float64.  A sigmoid's argument reaches |sdf| beta = 150 and carries 150 x 2^-24 = 1e-5 of rounding, which the
    sigmoid hands on as a relative error of its value (or of 1 - value) and the quotient to alpha; the product of up to 353 factors
    adds 353 x 2^-24 = 2e-5.  The gradients multiply by beta and by 1 / (c + eps) <= 1e5 x c, errors of the same relative size.  The
    bound is ten times their sum."""
    for beta, rho, with_normals, C in ((300.0, 0.3, True, 3), (20.0, 1.0, False, 1)):
        c, args = _variant(beta, rho, with_normals, C)
        f64, chain = reference.render_all_f64(c, *args), reference.render_chain(c, *args)
        assert sorted(f64) == sorted(chain)
        for name, truth in f64.items():
            err = np.abs(chain[name] - truth).max() / np.abs(truth).max()
            print("%s beta %g: float32 op chain %.3e" % (name, beta, err))
            assert chain[name].shape == truth.shape and err <= 3e-4, (name, beta, err)


# ---------------------------------------------------------------------------------------------------------------- PyTorch parts
def test_formulas_and_modules_on_cpu_tensors():
    from gaussianip_amd.utils.sdf_volume import ImplicitSDF, LearnedVariance, neus_alpha, volsdf_density
    from gaussianip_amd.utils.volume import OccupancyGrid
    g = torch.Generator().manual_seed(5)
    sdf = (torch.rand(200, generator=g, dtype=torch.float64) - 0.5) * 0.2
    d = torch.nn.functional.normalize(torch.randn(200, 3, generator=g, dtype=torch.float64), dim=-1)
    n = torch.nn.functional.normalize(torch.randn(200, 3, generator=g, dtype=torch.float64), dim=-1)
    dists = torch.rand(200, generator=g, dtype=torch.float64) * 0.01
    for rho in (1.0, 0.3, 0.0):
        assert torch.equal(neus_alpha(sdf, n, d, dists, 50.0, rho), reference.ref_alpha(sdf, n, d, dists, 50.0, rho))
    # the alpha_fn form by hand (neus_volume_renderer.py:135-141)
    step = 0.01
    c, m = torch.sigmoid((sdf + step * 0.5) * 50.0), torch.sigmoid((sdf - step * 0.5) * 50.0)
    assert torch.allclose(neus_alpha(sdf, None, None, step, 50.0), ((c - m + 1e-5) / (c + 1e-5)).clip(0, 1), rtol=1e-13, atol=0)
    a = neus_alpha(sdf, n, d, dists, 50.0)
    assert float(a.min()) >= 0 and float(a.max()) <= 1 and float(a.max()) > 0.05
    # VolSDF: inv_std x the Laplace CDF of -sdf
    lap = torch.where(sdf > 0, 0.5 * torch.exp(-sdf * 50.0), 1 - 0.5 * torch.exp(sdf * 50.0))
    assert torch.allclose(volsdf_density(sdf, torch.tensor(50.0, dtype=torch.float64)), 50.0 * lap, rtol=1e-12, atol=0)

    variance = LearnedVariance(0.3)
    assert [k for k, _ in variance.named_parameters()] == ["_inv_std"] and abs(float(variance.inv_std.detach()) - np.exp(3.0)) < 1e-4
    x = torch.zeros(4, 1)
    assert variance(x).shape == (4, 1) and torch.allclose(variance(x), torch.full((4, 1), float(np.exp(3.0))))
    assert float(LearnedVariance(2.0)(x)[0, 0]) == 1e6 and float(LearnedVariance(-2.0)(x)[0, 0]) == pytest.approx(1e-6)
    variance(x).sum().backward()
    assert float(variance._inv_std.grad) == pytest.approx(40 * np.exp(3.0), rel=1e-5)

    pts = torch.tensor([[0.0, 0.0, 0.0], [0.3, -0.4, 0.0], [1.0, 1.0, 1.0]], dtype=torch.float64)
    net = torch.tensor([[0.5], [-2.0], [1.0]], dtype=torch.float64)
    r = pts.norm(dim=-1, keepdim=True)
    for kwargs, expected in ((dict(sdf_bias=0.25), torch.full_like(r, 0.25)), (dict(sdf_bias="sphere", sdf_bias_params=0.5), r - 0.5),
                             (dict(sdf_bias="ellipsoid", sdf_bias_params=[0.5, 1.0, 2.0]),
                              ((pts / torch.tensor([0.5, 1.0, 2.0])) ** 2).sum(-1, keepdim=True).sqrt() - 1)):
        geometry = ImplicitSDF(pos_encoding_config=SMALL_GRID, **kwargs)
        assert torch.allclose(geometry.get_shifted_sdf(pts, net), net + expected, rtol=1e-12, atol=0), kwargs
    geometry = ImplicitSDF(radius=2.0, n_feature_dims=5, normal_type="pred", pos_encoding_config=SMALL_GRID)
    assert geometry.bbox.tolist() == [[-2.0] * 3, [2.0] * 3] and geometry.feature_network.layers[-1].out_features == 5
    assert geometry.normal_network.layers[-1].out_features == 3 and geometry.sdf_network.layers[-1].out_features == 1
    assert torch.equal(geometry.forward_level(net, 0.5), net - 0.5) and geometry.finite_difference_normal_eps == 0.01
    assert not hasattr(ImplicitSDF(n_feature_dims=0, pos_encoding_config=SMALL_GRID), "feature_network")
    for bad in (dict(normal_type="analytic"), dict(sdf_bias="blob"), dict(sdf_bias="sphere"), dict(radius=0.0),
                dict(finite_difference_normal_eps="progressive"), dict(finite_difference_normal_eps=0.0)):
        with pytest.raises(ValueError):
            ImplicitSDF(pos_encoding_config=SMALL_GRID, **bad)
    with pytest.raises(NotImplementedError):
        ImplicitSDF(pos_encoding_config=SMALL_GRID, shape_init="mesh:a.obj", shape_init_params=0.5).initialize_shape()
    ImplicitSDF(pos_encoding_config=SMALL_GRID).initialize_shape()  # no shape_init: nothing to do

    grid = OccupancyGrid([-1, -1, -1, 1, 1, 1], resolution=8)
    with pytest.raises(ValueError, match="not both"):
        grid.sampling(torch.zeros(4, 3), torch.ones(4, 3), sigma_fn=lambda *a: None, alpha_fn=lambda *a: None, render_step_size=0.1)


def test_progressive_finite_difference_eps_follows_the_grid():
    """finite_difference_normal_eps="progressive" (Neuralangelo's): update_step opens the ProgressiveBandHashGrid's levels and sets eps
    to the cell size of the finest open level, 2 radius / (base_resolution per_level_scale^(level - 1)), the level being
    min(start_level + max(step - start_step, 0) // update_steps, n_levels)."""
    from gaussianip_amd.utils.sdf_volume import ImplicitSDF
    config = {"otype": "ProgressiveBandHashGrid", "n_levels": 4, "n_features_per_level": 2, "log2_hashmap_size": 6, "base_resolution": 4,
              "per_level_scale": 1.5, "start_level": 2, "start_step": 10, "update_steps": 5}
    geometry = ImplicitSDF(radius=1.5, pos_encoding_config=config, finite_difference_normal_eps="progressive")
    band = geometry.encoding.encoding
    assert geometry.finite_difference_normal_eps is None and not band.mask.any()
    with pytest.raises(ValueError, match="update_step"):
        geometry(torch.zeros(2, 3), output_normal=True)
    for step, level in ((0, 2), (10, 2), (14, 2), (15, 3), (21, 4), (1000, 4)):
        geometry.update_step(step)
        assert band.current_level == level and int(band.mask.sum()) == 2 * level, step
        assert geometry.finite_difference_normal_eps == pytest.approx(2 * 1.5 / (4 * 1.5 ** (level - 1)), rel=1e-12), step
    # a fixed eps stays what it was given as, and a predicted normal needs none
    fixed = ImplicitSDF(pos_encoding_config=config, finite_difference_normal_eps=0.02)
    fixed.update_step(15)
    assert fixed.finite_difference_normal_eps == 0.02 and fixed.encoding.encoding.current_level == 3
    pred = ImplicitSDF(pos_encoding_config=config, normal_type="pred", finite_difference_normal_eps="progressive")
    pred.update_step(15)
    assert pred.finite_difference_normal_eps is None


# ---------------------------------------------------------------------------------------------------------------- pruning
def test_few_pruning_samples_are_undecided():
    """The GPU pruning test lets a sample go either way when, in float64, |alpha - alpha_thre| <= 1e-5 or |trans - early_stop_eps| <=
    1e-4 early_stop_eps: on its inputs at most 1 % of the samples are that close, and both outcomes occur among the rest."""
    p = inputs.pruning()
    _, trans = reference.weights_from_alpha_f64(p["alphas"], p["offsets"])
    alphas = p["alphas"].astype(np.float64)
    undecided = (np.abs(alphas - inputs.ALPHA_THRE) <= 1e-5) | (np.abs(trans - inputs.EARLY_STOP_EPS) <= 1e-4 * inputs.EARLY_STOP_EPS)
    keep = (alphas >= inputs.ALPHA_THRE) & (trans >= inputs.EARLY_STOP_EPS)
    M = trans.shape[0]
    print("pruning inputs: %d samples, %d undecided, %d kept" % (M, int(undecided.sum()), int(keep.sum())))
    assert M > 5000 and undecided.sum() <= 0.01 * M
    assert (alphas < inputs.ALPHA_THRE).sum() > 100 and (trans < inputs.EARLY_STOP_EPS).sum() > 100 and 100 < keep.sum() < M - 100


# ---------------------------------------------------------------------------------------------------------------- the entry points
def test_entry_points_check_their_arguments_and_launch_nothing():
    from gaussianip_amd import _lib
    lib = _lib.model_lib()
    one, null = ctypes.c_void_p(256), ctypes.c_void_p(None)         # never dereferenced: every call below fails or has nothing to do
    wf, wb = lib.gip_volume_alpha_weights_forward, lib.gip_volume_alpha_weights_backward
    assert wf(one, one, -1, 4, one, one, null) == 1 and wf(one, one, 4, -1, one, one, null) == 1 and wf(one, one, 4, 1 << 31, one, one, null) == 1
    assert wf(one, one, (1 << 31) // 64 + 1, 4, one, one, null) == 1
    for k in range(4):
        assert wf(*[null if j == k else one for j in range(2)], 4, 4, *[null if j + 2 == k else one for j in range(2)], null) == 1
    assert wf(null, null, 0, 0, null, null, null) == 0 and wf(null, one, 4, 0, null, null, null) == 0 and wf(null, null, 0, 4, null, null, null) == 0
    assert wb(one, one, one, one, -1, 4, one, null) == 1 and wb(one, one, one, one, 4, 1 << 31, one, null) == 1
    for k in range(5):
        p = [null if j == k else one for j in range(5)]
        assert wb(*p[:4], 4, 4, p[4], null) == 1
    assert wb(null, null, null, null, 0, 4, null, null) == 0 and wb(null, null, null, null, 4, 0, null, null) == 0

    def fwd(R=4, M=4, C=3, rho=1.0, ins=(one,) * 8, outs=(one,) * 4):
        return lib.gip_volume_sdf_render_forward(*ins, rho, R, M, C, *outs, null)

    def bwd(R=4, M=4, C=3, rho=1.0, ins=(one,) * 8, saved=(one,) * 3, g_in=(one, one), outs=(one,) * 4):
        return lib.gip_volume_sdf_render_backward(*ins, rho, *saved, *g_in, R, M, C, *outs, null)
    no_values = (one,) * 5 + (null, one, one)
    for fn in (fwd, bwd):
        assert fn(R=-1) == 1 and fn(M=-1) == 1 and fn(M=1 << 31) == 1 and fn(R=(1 << 31) // 64 + 1) == 1
        assert fn(C=-1) == 1 and fn(C=17) == 1 and fn(M=1 << 28, C=16) == 1 and fn(C=0) == 1 and fn(C=3, ins=no_values) == 1
        for rho in (-0.1, 1.5, float("nan"), float("inf")):
            assert fn(rho=rho) == 1
        for k in (0, 2, 3, 4, 6, 7):                                 # normals (1) and values (5) may be NULL
            assert fn(ins=tuple(null if j == k else one for j in range(8))) == 1, k
        for k in range(4):
            required = fn is fwd or k in (0, 3)                      # g_normals and g_values may be NULL
            if required:
                assert fn(outs=tuple(null if j == k else one for j in range(4))) == 1, k
        assert fn(R=0) == 0 and fn(M=0) == 0 and fn(R=0, M=0, C=0, ins=(null,) * 8, outs=(null,) * 4) == 0
    for k in range(3):
        assert bwd(saved=tuple(null if j == k else one for j in range(3))) == 1
    assert bwd(g_in=(null, one)) == 1
    assert bwd(ins=(one, null) + (one,) * 6) == 1                    # g_normals without normals


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_sdf_volume_kernels_do_not_spill(tmp_path):
    scratch, spilled, log = resource_usage("volume_sdf.hip", tmp_path / "o.o")
    for kernel in KERNELS:
        assert any(kernel in n for n in scratch), "no kernel-resource-usage remark for %s: %s" % (kernel, log[-500:])
    assert len(scratch) == len(KERNELS), sorted(scratch)
    bad = [(n, scratch[n], spilled.get(n, 0)) for n in scratch if scratch[n] or spilled.get(n, 0)]
    assert not bad, "kernels spilling: %s" % bad
