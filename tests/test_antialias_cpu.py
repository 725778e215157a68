"""The antialiasing mode on the host side: C-ABI layout of the new config field, the Python surface (settings, pipeline
parameters), the float64 compensation reference, and the composite oracle reference the GPU tests compare against."""
import ctypes
import os
import subprocess
from argparse import ArgumentParser

import numpy as np
import pytest
import torch

from antialias_reference import compensation, composite_grads, effective_opacities
from dense_reference import _quat_to_rot, dense_render, look_at_camera, random_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_config_field_offset_in_ctypes_and_c(tmp_path):
    from gaussianip_amd import _lib
    assert _lib.GipRasterConfig.antialiasing.offset == 188
    assert ctypes.sizeof(_lib.GipRasterConfig) == 192
    assert _lib.GipRasterConfig().antialiasing == 0                  # ctypes zero-fills: an older caller gets the fork's model
    src = tmp_path / "off.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gip_raster.h"\n'
                   'int main(void) { printf("%zu %zu %d\\n", offsetof(GipRasterConfig, antialiasing), sizeof(GipRasterConfig), '
                   'GIP_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "off"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == ["188", "192", "4"]


def test_library_abi_version_is_unchanged():
    from gaussianip_amd import _lib
    try:
        lib = _lib.raster_lib()
    except ImportError:
        pytest.skip("libgip_raster.so not built")
    assert lib.gip_abi_version() == 4


def test_settings_and_pipeline_params_surface():
    from gaussianip_amd import GaussianRasterizationSettings
    from gaussianip_amd.arguments import PipelineParams
    fork = dict(image_height=8, image_width=8, tanfovx=0.5, tanfovy=0.5, bg=torch.zeros(3), scale_modifier=1.0,
                viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0, campos=torch.zeros(3), prefiltered=False,
                debug=False)
    s = GaussianRasterizationSettings(**fork)
    assert s.antialiasing is False and len(s) == 13
    assert GaussianRasterizationSettings(*fork.values()).antialiasing is False
    assert GaussianRasterizationSettings(**fork, antialiasing=True).antialiasing is True
    assert GaussianRasterizationSettings(*fork.values(), True).antialiasing is True
    assert PipelineParams().antialiasing is False
    assert PipelineParams(antialiasing=True).antialiasing is True
    p = ArgumentParser()
    pp = PipelineParams(p)
    assert pp.antialiasing is False
    assert pp.extract(p.parse_args(["--antialiasing"])).antialiasing is True
    assert pp.extract(p.parse_args([])).antialiasing is False


def test_dropin_package_accepts_the_field():
    import importlib
    import sys
    sys.path.insert(0, os.path.join(ROOT, "gaussianip_amd", "dropin"))
    try:
        dgr = importlib.import_module("diff_gaussian_rasterization")
    finally:
        sys.path.pop(0)
    assert "antialiasing" in dgr.GaussianRasterizationSettings._fields
    assert dgr.GaussianRasterizationSettings._field_defaults["antialiasing"] is False


def _scene(P, seed, H, W, cam=(10.0, 40.0, 1.6, 60.0), **kw):
    sc = random_scene(P, seed, **kw)
    view, proj, campos, tanx, tany = look_at_camera(*cam, H, W)
    return sc, view, proj, campos, tanx, tany


def test_compensation_is_at_most_one_and_tends_to_one_for_large_gaussians():
    H = W = 64
    sc, view, proj, campos, tanx, tany = _scene(200, 5, H, W, scale_lo=0.001, scale_hi=0.05)
    comp = compensation(means3D=sc["means3D"], viewmatrix=view, H=H, W=W, tanfovx=tanx, tanfovy=tany, scales=sc["scales"],
                        rotations=sc["rotations"])
    assert comp.shape == (200,)
    assert bool((comp <= 1.0).all()) and bool((comp >= 0.005 - 1e-15).all())
    assert float(comp.min()) < 0.5                                        # sub-pixel splats lose opacity
    big = compensation(means3D=sc["means3D"], viewmatrix=view, H=H, W=W, tanfovx=tanx, tanfovy=tany,
                       scales=sc["scales"] * 0 + 0.5, rotations=sc["rotations"])
    assert float(big.min()) > 0.99
    # a needle (two vanishing axes): det of the undilated covariance ~ 0 -> clamped at sqrt(0.000025)
    needle = compensation(means3D=sc["means3D"][:4], viewmatrix=view, H=H, W=W, tanfovx=tanx, tanfovy=tany,
                          scales=torch.tensor([[0.05, 1e-9, 1e-9]] * 4, dtype=torch.float64), rotations=sc["rotations"][:4])
    assert torch.allclose(needle, torch.full((4,), 0.005, dtype=torch.float64))


def test_compensation_gradcheck():
    H, W = 48, 64
    sc, view, proj, campos, tanx, tany = _scene(12, 6, H, W, scale_lo=0.002, scale_hi=0.03)
    # row 0 on the clamped branch: a needle (det of the undilated 2-D covariance ~ 0)
    sc["scales"][0] = torch.tensor([0.03, 1e-7, 1e-7], dtype=torch.float64)
    sc["rotations"][0] = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64)
    args = [sc["means3D"].clone().requires_grad_(True), sc["scales"].clone().requires_grad_(True),
            sc["rotations"].clone().requires_grad_(True)]

    def f(m, s, q):
        return compensation(means3D=m, viewmatrix=view, H=H, W=W, tanfovx=tanx, tanfovy=tany, scales=s, rotations=q)

    assert float(f(*args)[0].detach()) == pytest.approx(0.005)
    assert torch.autograd.gradcheck(f, args)
    g = torch.autograd.grad(f(*args)[0], args)
    assert all(float(t.abs().max()) == 0.0 for t in g)                     # clamped branch: the chain contributes zero
    R = _quat_to_rot(sc["rotations"])
    L = R * sc["scales"][:, None, :]
    S = L @ L.transpose(1, 2)
    cov = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], dim=1)[1:].clone().requires_grad_(True)
    m = sc["means3D"][1:].clone().requires_grad_(True)
    assert torch.autograd.gradcheck(
        lambda m_, c_: compensation(means3D=m_, viewmatrix=view, H=H, W=W, tanfovx=tanx, tanfovy=tany, cov3D_precomp=c_),
        [m, cov], eps=1e-9)


def _composite_vs_dense(oracle, P, H, W, seed, sh_degree=0, use_cov=False, use_colors=False, bgval=(0.2, 0.5, 0.9),
                        cam=(10.0, 40.0, 1.6, 60.0), scene_kw=None, fork_clamp=False):
    M = (sh_degree + 1) ** 2
    sc64, view, proj, campos, tanx, tany = _scene(P, seed, H, W, cam=cam, sh_M=M, **(scene_kw or dict(scale_lo=0.004, scale_hi=0.05)))
    sc = {k: v.numpy().astype(np.float32) for k, v in sc64.items()}
    scd = {k: torch.from_numpy(v).double() for k, v in sc.items()}          # the float32 scene, exactly, in float64
    bg = torch.tensor(bgval, dtype=torch.float64)
    cam = dict(viewmatrix=view.numpy().astype(np.float32), projmatrix=proj.numpy().astype(np.float32),
               campos=campos.numpy().astype(np.float32), tanfovx=tanx, tanfovy=tany)
    camd = {k: (torch.from_numpy(v).double() if isinstance(v, np.ndarray) else v) for k, v in cam.items()}
    cov = None
    leaves = {k: scd[k].clone().requires_grad_(True) for k in ("means3D", "opacities")}
    ckw = {}
    okw = dict(image_height=H, image_width=W, tanfovx=tanx, tanfovy=tany, bg=bg.numpy().astype(np.float32), scale_modifier=1.0,
               viewmatrix=cam["viewmatrix"], projmatrix=cam["projmatrix"], sh_degree=sh_degree, campos=cam["campos"],
               means3D=sc["means3D"])
    if use_cov:
        R = _quat_to_rot(scd["rotations"])
        L = R * scd["scales"][:, None, :]
        S = L @ L.transpose(1, 2)
        cov = torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], dim=1).float().double()
        leaves["cov3D_precomp"] = cov.clone().requires_grad_(True)
        ckw["cov3D_precomp"] = leaves["cov3D_precomp"]
        okw["cov3D_precomp"] = cov.numpy().astype(np.float32)
    else:
        for k in ("scales", "rotations"):
            leaves[k] = scd[k].clone().requires_grad_(True)
            ckw[k] = leaves[k]
            okw[k] = sc[k]
    if use_colors:
        col = torch.rand(P, 3, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64).float().double()
        leaves["colors_precomp"] = col.clone().requires_grad_(True)
        okw["colors_precomp"] = col.numpy().astype(np.float32)
    else:
        leaves["shs"] = scd["shs"].clone().requires_grad_(True)
        okw["shs"] = sc["shs"]
    # dense float64 antialiased model
    comp = compensation(means3D=leaves["means3D"], viewmatrix=camd["viewmatrix"], H=H, W=W, tanfovx=tanx, tanfovy=tany,
                        fork_clamp=fork_clamp, **ckw)
    m2d = torch.zeros(P, 3, dtype=torch.float64, requires_grad=True)
    out = dense_render(means3D=leaves["means3D"], opacities=leaves["opacities"] * comp[:, None], viewmatrix=camd["viewmatrix"],
                       projmatrix=camd["projmatrix"], campos=camd["campos"], bg=bg, H=H, W=W, tanfovx=tanx, tanfovy=tany,
                       sh_degree=sh_degree, means2D=m2d, shs=leaves.get("shs"), colors_precomp=leaves.get("colors_precomp"),
                       scales=leaves.get("scales"), rotations=leaves.get("rotations"), cov3D_precomp=leaves.get("cov3D_precomp"),
                       fork_clamp=fork_clamp)
    g = torch.Generator().manual_seed(99)
    gC = torch.randn(3, H, W, generator=g, dtype=torch.float64)
    gD = torch.randn(1, H, W, generator=g, dtype=torch.float64)
    gA = torch.randn(1, H, W, generator=g, dtype=torch.float64)
    ((out["color"] * gC).sum() + (out["depth"] * gD).sum() + (out["alpha"] * gA).sum()).backward()
    # composite oracle reference: forward on the effective opacities, backward chained through comp
    comp_np = comp.detach()
    ro = oracle.RasterOracle()
    color, radii, depth, alpha = ro.forward(opacities=effective_opacities(sc, comp_np), **okw)
    assert np.array_equal(radii, out["radii"].numpy())
    np.testing.assert_allclose(color, out["color"].detach().numpy(), atol=2e-5)
    np.testing.assert_allclose(depth, out["depth"].detach().numpy(), atol=2e-5)
    np.testing.assert_allclose(alpha, out["alpha"].detach().numpy(), atol=2e-5)
    go = ro.backward(gC.numpy(), gD.numpy(), gA.numpy())
    ref = composite_grads(go, sc, cam, H, W, cov=None if cov is None else cov.numpy(), fork_clamp=fork_clamp)

    def close(name, ours, dense, tol=2e-3):
        dense = dense.detach().numpy().reshape(np.shape(ours))
        err = np.abs(ours - dense).max() / (np.abs(dense).max() + 1e-12)
        assert err < tol, "%s: rel-to-max error %.3e" % (name, err)

    close("means2D", ref["means2D"][:, :2], m2d.grad[:, :2])
    for k, v in leaves.items():
        close(k, ref[k], v.grad)
    return comp_np


@pytest.mark.parametrize("deg", [0, 1, 3])
def test_composite_oracle_reference_equals_dense_antialiased_model(oracle, deg):
    comp = _composite_vs_dense(oracle, P=120, H=48, W=56, seed=40 + deg, sh_degree=deg)
    assert float(comp.min()) < 0.9          # the mode changes this scene


def test_composite_oracle_reference_on_clamped_gaussians(oracle):
    """Scene A of test_oracle_vs_dense.py (48 visible Gaussians on the clamped side of the Jacobian, 24 behind the near plane):
    the compensation's derivative runs through the clamped Jacobian too, so the composite reference and the dense model take
    `fork_clamp` alike.  The reference of test_gpu_raster_branches.py's antialiased case."""
    from dense_reference import clamp_cull_masks
    from test_oracle_vs_dense import SCENE_A as A
    comp = _composite_vs_dense(oracle, P=A["P"], H=A["H"], W=A["W"], seed=A["seed"], sh_degree=A["sh_degree"], cam=A["cam"],
                               scene_kw=A["scene_kw"], fork_clamp=True)
    sc, view, _, _, tanx, tany = _scene(A["P"], A["seed"], A["H"], A["W"], cam=A["cam"], **A["scene_kw"])
    clamped, behind = clamp_cull_masks(sc["means3D"].numpy(), view.numpy(), tanx, tany)
    # the compensation must act on the clamped Gaussians, or their branch of its derivative carries nothing
    assert int((clamped & (comp.numpy() < 0.999)).sum()) >= 24 and int(behind.sum()) >= 12


def test_composite_oracle_reference_equals_dense_precomputed_inputs(oracle):
    _composite_vs_dense(oracle, P=100, H=48, W=48, seed=47, use_cov=True, use_colors=True)
