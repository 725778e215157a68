"""Float64 PyTorch restatement of the antialiasing mode's opacity compensation (GaussianRasterizationSettings.antialiasing).

With the mode on, every (view, Gaussian) blends with opacity * comp, where, from the projected 2-D covariance (a0, b, c0)
before the +0.3 px^2 dilation,
    comp = sqrt(max(0.000025, (a0 c0 - b^2) / ((a0 + 0.3) (c0 + 0.3) - b^2)))
and everything else (conic, radius, tile rectangle) is the fork's.  The projection follows tests/dense_reference.py
(same 1.3 tanfov clamp of J), so the dense antialiased render is dense_render(..., opacities=opacities * comp[:, None]).

`composite_oracle` builds the same model from the C oracle (oracle/raster_oracle.c), which knows nothing of the mode: its
forward on opacities * comp, and its backward (gradient w.r.t. that effective opacity) chained through the autograd of
comp here.  tests/test_antialias_cpu.py pins this composite against the dense model; the GPU tests use it at sizes the
dense model cannot reach.
"""
import numpy as np
import torch

from dense_reference import _quat_to_rot

COMP_MIN = 0.000025
DILATION = 0.3


def compensation(*, means3D, viewmatrix, H, W, tanfovx, tanfovy, scales=None, rotations=None, cov3D_precomp=None,
                 scale_modifier=1.0, fork_clamp=False):
    """comp [P] (float64) for one view; differentiable in means3D and in scales / rotations or cov3D_precomp.
    viewmatrix: [4,4] in the cameras.py layout (row-vector convention).  Values of Gaussians behind the near plane are
    finite but meaningless (the rasterizer culls them).  `fork_clamp`: as in dense_reference.dense_render (comp's derivative
    runs through the same clamped Jacobian as the conic's)."""
    dt = torch.float64
    P = means3D.shape[0]
    ph = torch.cat([means3D, torch.ones(P, 1, dtype=dt)], dim=1)
    pv = ph @ viewmatrix
    tz = pv[:, 2]
    if cov3D_precomp is not None:
        c = cov3D_precomp
        Sigma = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], dim=-1).reshape(-1, 3, 3)
    else:
        R = _quat_to_rot(rotations)
        L = R * (scale_modifier * scales)[:, None, :]
        Sigma = L @ L.transpose(1, 2)
    fx = W / (2.0 * tanfovx)
    fy = H / (2.0 * tanfovy)
    limx, limy = 1.3 * tanfovx, 1.3 * tanfovy
    tzs = torch.where(tz > 0.2, tz, torch.ones_like(tz))
    tx = torch.clamp(pv[:, 0] / tzs, -limx, limx) * tzs
    ty = torch.clamp(pv[:, 1] / tzs, -limy, limy) * tzs
    if fork_clamp:
        tx = torch.where((pv[:, 0] / tzs).abs() > limx, tx.detach(), pv[:, 0])
        ty = torch.where((pv[:, 1] / tzs).abs() > limy, ty.detach(), pv[:, 1])
    zero = torch.zeros_like(tzs)
    J = torch.stack([fx / tzs, zero, -(fx * tx) / (tzs * tzs), zero, fy / tzs, -(fy * ty) / (tzs * tzs)], dim=-1).reshape(-1, 2, 3)
    Mx = J @ viewmatrix[:3, :3].transpose(0, 1)
    cov2 = Mx @ Sigma @ Mx.transpose(1, 2)
    a0, b, c0 = cov2[:, 0, 0], cov2[:, 0, 1], cov2[:, 1, 1]
    det0 = a0 * c0 - b * b
    det1 = (a0 + DILATION) * (c0 + DILATION) - b * b
    return torch.sqrt(torch.clamp_min(det0 / det1, COMP_MIN))


def _t64(a):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=torch.float64)


def scene_compensation(sc, cam, H, W, cov=None, requires_grad=False, fork_clamp=False):
    """comp of a numpy scene (tests/scenes.py layout) under a numpy camera (scenes.camera): returns (comp [P] float64 tensor,
    leaves dict).  With requires_grad the leaves (means3D and scales / rotations, or cov3D_precomp) are autograd leaves."""
    leaves = {"means3D": _t64(sc["means3D"])}
    if cov is None:
        leaves.update(scales=_t64(sc["scales"]), rotations=_t64(sc["rotations"]))
    else:
        leaves["cov3D_precomp"] = _t64(cov)
    if requires_grad:
        for v in leaves.values():
            v.requires_grad_(True)
    comp = compensation(viewmatrix=_t64(cam["viewmatrix"]), H=H, W=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
                        fork_clamp=fork_clamp, **leaves)
    return comp, leaves


def effective_opacities(sc, comp):
    """float32 [P,1] opacity the oracle blends with in the antialiased model."""
    return (np.asarray(sc["opacities"], np.float64) * comp.detach().numpy()[:, None]).astype(np.float32)


def composite_grads(go, sc, cam, H, W, cov=None, fork_clamp=False):
    """Every gradient of the antialiased model from an oracle backward `go` run on effective opacities:
    dL/dopacity = comp * dL/dopacity_eff, and dL/dopacity_eff * opacity chained through comp into means3D and
    scales / rotations (or cov3D_precomp).  Returns a dict shaped like `go` (float64)."""
    comp, leaves = scene_compensation(sc, cam, H, W, cov=cov, requires_grad=True, fork_clamp=fork_clamp)
    g_eff = np.asarray(go["opacities"], np.float64).reshape(-1)
    w = torch.from_numpy(g_eff * np.asarray(sc["opacities"], np.float64).reshape(-1))
    names = list(leaves)
    extra = torch.autograd.grad(comp, [leaves[n] for n in names], grad_outputs=w)
    out = {k: np.asarray(v, np.float64) for k, v in go.items() if v is not None}
    out["opacities"] = (g_eff * comp.detach().numpy()).reshape(np.shape(go["opacities"]))
    for n, e in zip(names, extra):
        key = "cov3D_precomp" if n == "cov3D_precomp" else n
        out[key] = out[key] + e.numpy().reshape(out[key].shape)
    return out
