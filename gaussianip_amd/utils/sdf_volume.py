"""NeuS volume rendering of a signed-distance field (csrc/volume_sdf.hip, gip_volume_alpha_weights_* and gip_volume_sdf_render_*): what
the reference's neus-volume-renderer (threestudio/models/renderers/neus_volume_renderer.py) and its implicit-sdf geometry
(threestudio/models/geometry/implicit_sdf.py) need next to utils/volume.py, which marches the rays.  nerfacc is CUDA-only; the
definition is the kernel file's header, the project's own, and has not been compared with nerfacc's output.

  render_weight_from_alpha(alphas, ray_indices, n_rays)     (weights, trans); gradient to alphas, finite at alpha == 1.  First order only.
  neus_alpha, volsdf_density                                the reference's formulas as PyTorch ops: the op chain, VolSDF, the CPU
  render_sdf_rays(sdf, normals, rays_d, t_starts, t_ends, values, inv_std, ray_indices, n_rays, cos_anneal_ratio)
                                   (out [R, 2 + C] = opacity, depth, channels; weights; alphas): SDF -> alpha -> weights -> the sums
                                   along every ray in ONE launch, and their backward in one.  First order only.
  LearnedVariance                  the reference's: inv_std = exp(10 _inv_std)
  ImplicitSDF                      the reference's implicit-sdf geometry over get_encoding / get_mlp; isosurface() hands it to the
                                   tetrahedral stage (utils/isosurface.py)
  NeuSVolumeRenderer               the reference's neus-volume-renderer with the no-material and a solid background

Every kernel output is bitwise equal from run to run: nothing is summed with atomics.  There is no CPU path for the kernels: their
inputs are float32 GPU tensors, anything else raises ValueError.  neus_alpha, volsdf_density, LearnedVariance and the geometry's
bias are plain PyTorch and run wherever their tensors live."""
import math

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from .._lib import call_model, ptr
from .encoding import get_encoding, get_mlp
from .volume import (MAX_CHANNELS, _INT32_MAX, OccupancyGrid, _background, _chunked, _is_f32_gpu, _offsets, accumulate_along_rays)

__all__ = ["render_weight_from_alpha", "neus_alpha", "volsdf_density", "render_sdf_rays", "LearnedVariance", "ImplicitSDF", "NeuSVolumeRenderer"]

EPS = 1e-5


class _AlphaWeights(torch.autograd.Function):
    @staticmethod
    def forward(ctx, alphas, offsets, R):
        dev, M = alphas.device, int(alphas.shape[0])
        a = alphas.detach().contiguous()
        with torch.cuda.device(dev):
            weights, trans = (torch.zeros(M, dtype=torch.float32, device=dev) for _ in range(2))
            if M and R:
                call_model(dev, "gip_volume_alpha_weights_forward", ptr(a), ptr(offsets), R, M, ptr(weights), ptr(trans))
        ctx.save_for_backward(a, trans, offsets)
        ctx.R = R
        ctx.mark_non_differentiable(trans)
        return weights, trans

    @staticmethod
    @once_differentiable
    def backward(ctx, g_weights, _g_trans):
        a, trans, offsets = ctx.saved_tensors
        dev, M = a.device, int(a.shape[0])
        g = g_weights.contiguous().float()
        with torch.cuda.device(dev):
            g_alphas = torch.zeros(M, dtype=torch.float32, device=dev)
            if M and ctx.R:
                call_model(dev, "gip_volume_alpha_weights_backward", ptr(a), ptr(trans), ptr(g), ptr(offsets), ctx.R, M, ptr(g_alphas))
        return g_alphas, None, None


def render_weight_from_alpha(alphas, ray_indices=None, n_rays=None):
    """(weights, trans) [M] of the opacities alphas [M]: trans = the product of 1 - alpha over the ray's earlier samples, weight =
    trans alpha.  nerfacc's name and argument order.  ray_indices [M] (sorted, as march_rays returns them) with n_rays, or neither for
    one ray.  Differentiable in alphas, first order only, by a recurrence without a division: the gradient is finite where an alpha
    is exactly 1.  trans carries no gradient.  Bitwise reproducible, forward and backward."""
    if not _is_f32_gpu(alphas, 1):
        raise ValueError("render_weight_from_alpha: alphas must be an [M] float32 GPU tensor")
    offsets, _, R = _offsets("render_weight_from_alpha", ray_indices, n_rays, int(alphas.shape[0]), alphas.device)
    return _AlphaWeights.apply(alphas, offsets, R)


def volsdf_density(sdf, inv_std):
    """The reference's volsdf_density (:17-20): the Laplace CDF of -sdf with scale 1 / inv_std, times inv_std."""
    beta = 1 / inv_std
    return inv_std * (0.5 + 0.5 * sdf.sign() * torch.expm1(-sdf.abs() / beta))


def neus_alpha(sdf, normal, dirs, dists, inv_std, cos_anneal_ratio=1.0):
    """The reference's get_alpha with use_volsdf off (:77-95) as PyTorch ops: alpha of the signed distances sdf [...] with the normals
    normal [..., 3], the ray directions dirs [..., 3] and the sample lengths dists [...]; inv_std a number or a tensor that broadcasts
    against sdf.  normal None is the form of the reference's alpha_fn and occ_eval_fn (:135-141), iter_cos = -1, dirs unused."""
    if normal is None:
        iter_cos = -1.0
    else:
        true_cos = (dirs * normal).sum(-1)
        iter_cos = -(torch.relu(-true_cos * 0.5 + 0.5) * (1.0 - cos_anneal_ratio) + torch.relu(-true_cos) * cos_anneal_ratio)
    estimated_next_sdf = sdf + iter_cos * dists * 0.5
    estimated_prev_sdf = sdf - iter_cos * dists * 0.5
    prev_cdf = torch.sigmoid(estimated_prev_sdf * inv_std)
    next_cdf = torch.sigmoid(estimated_next_sdf * inv_std)
    return ((prev_cdf - next_cdf + EPS) / (prev_cdf + EPS)).clip(0.0, 1.0)


class _SdfRender(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sdf, normals, values, inv_std, rays_d, t_starts, t_ends, offsets, R, rho):
        dev, M = sdf.device, int(sdf.shape[0])
        C = 0 if values is None else int(values.shape[1])
        s, d, ts, te = (t.detach().contiguous() for t in (sdf, rays_d, t_starts, t_ends))
        n = None if normals is None else normals.detach().contiguous()
        v = None if values is None else values.detach().contiguous()
        beta = inv_std.detach().reshape(1).contiguous()
        with torch.cuda.device(dev):
            alphas, trans, weights = (torch.zeros(M, dtype=torch.float32, device=dev) for _ in range(3))
            out = torch.zeros((R, 2 + C), dtype=torch.float32, device=dev)
            if M and R:
                call_model(dev, "gip_volume_sdf_render_forward", ptr(s), ptr(n), ptr(d), ptr(ts), ptr(te), ptr(v), ptr(offsets), ptr(beta), rho,
                           R, M, C, ptr(alphas), ptr(trans), ptr(weights), ptr(out))
        ctx.save_for_backward(s, n, v, beta, d, ts, te, offsets, alphas, trans, weights)
        ctx.R, ctx.C, ctx.rho, ctx.beta_shape = R, C, rho, inv_std.shape
        ctx.mark_non_differentiable(alphas)
        ctx.set_materialize_grads(False)
        return out, weights, alphas

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out, g_weights, _g_alphas):
        s, n, v, beta, d, ts, te, offsets, alphas, trans, weights = ctx.saved_tensors
        dev, M, R, C = s.device, int(s.shape[0]), ctx.R, ctx.C
        need_n, need_v = n is not None and ctx.needs_input_grad[1], v is not None and ctx.needs_input_grad[2]
        with torch.cuda.device(dev):
            go = torch.zeros((R, 2 + C), dtype=torch.float32, device=dev) if g_out is None else g_out.contiguous().float()
            gw = None if g_weights is None else g_weights.contiguous().float()
            g_sdf = torch.zeros(M, dtype=torch.float32, device=dev)
            g_n = torch.zeros((M, 3), dtype=torch.float32, device=dev) if need_n else None
            g_v = torch.zeros((M, C), dtype=torch.float32, device=dev) if need_v else None
            g_rays = torch.zeros(R, dtype=torch.float32, device=dev)
            if M and R:
                call_model(dev, "gip_volume_sdf_render_backward", ptr(s), ptr(n), ptr(d), ptr(ts), ptr(te), ptr(v), ptr(offsets), ptr(beta),
                           ctx.rho, ptr(alphas), ptr(trans), ptr(weights), ptr(go), ptr(gw), R, M, C, ptr(g_sdf), ptr(g_n), ptr(g_v),
                           ptr(g_rays))
            g_beta = torch.sum(g_rays).reshape(ctx.beta_shape)
        return g_sdf, g_n, g_v, g_beta, None, None, None, None, None, None


def render_sdf_rays(sdf, normals, rays_d, t_starts, t_ends, values, inv_std, ray_indices, n_rays, cos_anneal_ratio=1.0):
    """(out [n_rays, 2 + C], weights [M], alphas [M]) of the signed distances sdf [M] at the samples (t_starts, t_ends) [M] of the rays
    with the directions rays_d [n_rays, 3]: alpha as neus_alpha gives it (normals [M, 3], or None for iter_cos = -1), weights as
    render_weight_from_alpha, and along every ray out[:, 0] = the sum of the weights (opacity), out[:, 1] = of weights x the samples'
    midpoints (depth), out[:, 2:] = of weights x values [M, C], C = 1 .. 16, or nothing for values None.  inv_std: a 1-element tensor,
    read on the device.  ray_indices [M] (sorted) with n_rays.  One launch forward and one backward.  Differentiable in sdf, normals,
    values and inv_std, first order only, through out and through weights; alphas carry no gradient, and the rays and the samples none
    either.  Bitwise reproducible, forward and backward; inv_std's gradient is the torch.sum of per-ray parts."""
    if not (_is_f32_gpu(sdf, 1) and _is_f32_gpu(t_starts, 1) and _is_f32_gpu(t_ends, 1) and t_starts.shape == t_ends.shape == sdf.shape and
            t_starts.device == t_ends.device == sdf.device):
        raise ValueError("render_sdf_rays: sdf, t_starts and t_ends must be [M] float32 GPU tensors on one device")
    dev, M = sdf.device, int(sdf.shape[0])
    if normals is not None and not (_is_f32_gpu(normals, 2) and normals.device == dev and tuple(normals.shape) == (M, 3)):
        raise ValueError("render_sdf_rays: normals must be an [M, 3] float32 GPU tensor on the samples' device, or None")
    if values is not None and not (_is_f32_gpu(values, 2) and values.device == dev and values.shape[0] == M and 1 <= values.shape[1] <= MAX_CHANNELS):
        raise ValueError("render_sdf_rays: values must be an [M, C] float32 GPU tensor on the samples' device, C = 1 .. %d, or None" % MAX_CHANNELS)
    if M * (1 if values is None else int(values.shape[1])) > _INT32_MAX:
        raise ValueError("render_sdf_rays: %d samples x channels do not fit 31 bits" % M)
    if not (isinstance(inv_std, torch.Tensor) and inv_std.is_cuda and inv_std.device == dev and inv_std.dtype == torch.float32 and inv_std.numel() == 1):
        raise ValueError("render_sdf_rays: inv_std must be a 1-element float32 GPU tensor on the samples' device")
    rho = float(cos_anneal_ratio)
    if not (math.isfinite(rho) and 0.0 <= rho <= 1.0):
        raise ValueError("render_sdf_rays: cos_anneal_ratio must lie in [0, 1]")
    if ray_indices is None:
        raise ValueError("render_sdf_rays: ray_indices and n_rays must be given")
    offsets, _, R = _offsets("render_sdf_rays", ray_indices, n_rays, M, dev)
    if not (_is_f32_gpu(rays_d, 2) and rays_d.device == dev and tuple(rays_d.shape) == (R, 3)):
        raise ValueError("render_sdf_rays: rays_d must be an [n_rays, 3] float32 GPU tensor on the samples' device")
    return _SdfRender.apply(sdf, normals, values, inv_std, rays_d, t_starts, t_ends, offsets, R, rho)


class LearnedVariance(nn.Module):
    """The reference's LearnedVariance (:23-34): the parameter _inv_std, inv_std = exp(10 _inv_std), forward(x) = inv_std clamped to
    [1e-6, 1e6] in the shape of x."""

    def __init__(self, init_val):
        super().__init__()
        self.register_parameter("_inv_std", nn.Parameter(torch.tensor(float(init_val))))

    @property
    def inv_std(self):
        return torch.exp(self._inv_std * 10.0)

    def forward(self, x):
        return torch.ones_like(x) * self.inv_std.clamp(1.0e-6, 1.0e6)


NORMAL_TYPES = ("finite_difference", "finite_difference_laplacian", "pred")


def _is_number(x):
    return isinstance(x, (int, float)) and not isinstance(x, bool)


class ImplicitSDF(nn.Module):
    """The reference's implicit-sdf geometry (threestudio/models/geometry/implicit_sdf.py): a position encoding over the box
    [-radius, radius]^3 with one MLP for the signed distance (inside is negative) and one for n_feature_dims features.  The
    configuration keys are keyword arguments; the encoding and MLP configurations default to the reference's (a 16-level hash grid, one
    hidden layer of 64).  sdf = network + bias, the bias a number, "sphere" (|x| - sdf_bias_params, a float) or "ellipsoid"
    (|x / sdf_bias_params| - 1, three semi-axes).  normal_type "analytic" needs second derivatives of the encoding, which is first
    order only: ValueError.  finite_difference_normal_eps: a number, or "progressive" (Neuralangelo's; needs a ProgressiveBandHashGrid
    and update_step).  shape_init "sphere" / "ellipsoid" with shape_init_params fits the field to that shape in initialize_shape();
    "mesh:..." needs trimesh and pysdf, which this project does not depend on: NotImplementedError."""

    POS_ENCODING_CONFIG = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
                           "per_level_scale": 1.447269237440378}
    MLP_NETWORK_CONFIG = {"otype": "VanillaMLP", "activation": "ReLU", "output_activation": "none", "n_neurons": 64, "n_hidden_layers": 1}

    def __init__(self, radius=1.0, n_feature_dims=3, pos_encoding_config=None, mlp_network_config=None, normal_type="finite_difference",
                 finite_difference_normal_eps=0.01, shape_init=None, shape_init_params=None, force_shape_init=False, sdf_bias=0.0,
                 sdf_bias_params=None):
        super().__init__()
        if not float(radius) > 0:
            raise ValueError("ImplicitSDF: radius must be positive")
        if normal_type not in NORMAL_TYPES:
            raise ValueError("ImplicitSDF: normal_type must be one of %s (the hash grid is first order only: no \"analytic\")" % (NORMAL_TYPES,))
        if not (_is_number(finite_difference_normal_eps) and finite_difference_normal_eps > 0) and finite_difference_normal_eps != "progressive":
            raise ValueError("ImplicitSDF: finite_difference_normal_eps must be a positive number or \"progressive\"")
        if sdf_bias == "sphere":
            if not _is_number(sdf_bias_params):
                raise ValueError("ImplicitSDF: sdf_bias 'sphere' needs a radius in sdf_bias_params")
        elif sdf_bias == "ellipsoid":
            if not (hasattr(sdf_bias_params, "__len__") and len(sdf_bias_params) == 3):
                raise ValueError("ImplicitSDF: sdf_bias 'ellipsoid' needs three semi-axes in sdf_bias_params")
        elif not _is_number(sdf_bias):
            raise ValueError("ImplicitSDF: unknown sdf bias %r" % (sdf_bias,))
        if shape_init is not None and not isinstance(shape_init, str):
            raise ValueError("ImplicitSDF: shape_init must be a string or None")
        self.radius, self.n_feature_dims = float(radius), int(n_feature_dims)
        self.normal_type = normal_type
        self.cfg_finite_difference_normal_eps = finite_difference_normal_eps
        self.finite_difference_normal_eps = float(finite_difference_normal_eps) if _is_number(finite_difference_normal_eps) else None
        self.shape_init, self.shape_init_params, self.force_shape_init = shape_init, shape_init_params, bool(force_shape_init)
        self.sdf_bias, self.sdf_bias_params = sdf_bias, sdf_bias_params
        self.register_buffer("bbox", torch.tensor([[-self.radius] * 3, [self.radius] * 3], dtype=torch.float32))
        self.pos_encoding_config = dict(self.POS_ENCODING_CONFIG if pos_encoding_config is None else pos_encoding_config)
        mlp = dict(self.MLP_NETWORK_CONFIG if mlp_network_config is None else mlp_network_config)
        if finite_difference_normal_eps == "progressive" and self.pos_encoding_config.get("otype") != "ProgressiveBandHashGrid":
            raise ValueError("ImplicitSDF: finite_difference_normal_eps=\"progressive\" only works with a ProgressiveBandHashGrid")
        self.encoding = get_encoding(3, self.pos_encoding_config)
        self.sdf_network = get_mlp(self.encoding.n_output_dims, 1, mlp)
        if self.n_feature_dims > 0:
            self.feature_network = get_mlp(self.encoding.n_output_dims, self.n_feature_dims, mlp)
        if normal_type == "pred":
            self.normal_network = get_mlp(self.encoding.n_output_dims, 3, mlp)
        self._helpers = {}

    def _unit(self, points):
        """The box mapped to [0, 1]^3: the reference's contract_to_unisphere(..., unbounded=False)."""
        return (points - self.bbox[0]) / (self.bbox[1] - self.bbox[0])

    def _encode(self, points):
        return self.encoding(self._unit(points).reshape(-1, 3))

    def get_shifted_sdf(self, points, sdf):
        """sdf [..., 1] plus the bias at points [..., 3] (world coordinates)."""
        if self.sdf_bias == "ellipsoid":
            size = torch.as_tensor(self.sdf_bias_params).to(points)
            bias = ((points / size) ** 2).sum(dim=-1, keepdim=True).sqrt() - 1.0
        elif self.sdf_bias == "sphere":
            bias = (points ** 2).sum(dim=-1, keepdim=True).sqrt() - float(self.sdf_bias_params)
        else:
            bias = float(self.sdf_bias)
        return sdf + bias

    def forward_sdf(self, points):
        """sdf [..., 1] at points [..., 3]."""
        return self.get_shifted_sdf(points, self.sdf_network(self._encode(points)).reshape(*points.shape[:-1], 1))

    def forward_field(self, points):
        """(sdf [..., 1], None): the field the isosurface is taken of, and no grid deformation."""
        return self.forward_sdf(points), None

    def forward_level(self, field, threshold):
        return field - threshold

    def forward(self, points, output_normal=False):
        """{"sdf" [..., 1], "features" [..., n_feature_dims] when there are any, and with output_normal "normal", "shading_normal" and
        "sdf_grad" [..., 3]} at points [..., 3]: the reference's dict."""
        if output_normal and self.normal_type != "pred" and self.finite_difference_normal_eps is None:
            raise ValueError("ImplicitSDF: finite_difference_normal_eps=\"progressive\" is set by update_step, which has not run")
        enc = self._encode(points)
        sdf = self.get_shifted_sdf(points, self.sdf_network(enc).view(*points.shape[:-1], 1))
        out = {"sdf": sdf}
        if self.n_feature_dims > 0:
            out["features"] = self.feature_network(enc).view(*points.shape[:-1], self.n_feature_dims)
        if output_normal:
            if self.normal_type == "pred":
                normal = nn.functional.normalize(self.normal_network(enc).view(*points.shape[:-1], 3), dim=-1)
                sdf_grad = normal
            else:
                eps = self.finite_difference_normal_eps
                if self.normal_type == "finite_difference_laplacian":
                    shifts = torch.tensor([[eps, 0, 0], [-eps, 0, 0], [0, eps, 0], [0, -eps, 0], [0, 0, eps], [0, 0, -eps]]).to(points)
                    moved = self.forward_sdf((points[..., None, :] + shifts).clamp(-self.radius, self.radius))
                    sdf_grad = 0.5 * (moved[..., 0::2, 0] - moved[..., 1::2, 0]) / eps
                else:
                    shifts = torch.tensor([[eps, 0, 0], [0, eps, 0], [0, 0, eps]]).to(points)
                    moved = self.forward_sdf((points[..., None, :] + shifts).clamp(-self.radius, self.radius))
                    sdf_grad = (moved[..., 0] - sdf) / eps
                normal = nn.functional.normalize(sdf_grad, dim=-1)
            out.update(normal=normal, shading_normal=normal, sdf_grad=sdf_grad)
        return out

    def update_step(self, global_step):
        """The reference's update_step: the encoding's own (a progressive band), and with finite_difference_normal_eps="progressive"
        the size of a cell of the finest level in use."""
        if hasattr(self.encoding, "update_step"):
            self.encoding.update_step(0, int(global_step))
        if self.normal_type == "pred" or self.cfg_finite_difference_normal_eps != "progressive":
            return
        cfg = self.pos_encoding_config
        level = min(cfg["start_level"] + max(int(global_step) - cfg["start_step"], 0) // cfg["update_steps"], cfg["n_levels"])
        self.finite_difference_normal_eps = 2 * self.radius / (cfg["base_resolution"] * cfg["per_level_scale"] ** (level - 1))

    def initialize_shape(self, steps=1000, batch=10000, lr=1e-3):
        """Fits the field to shape_init as the reference does (:91-218): `steps` Adam steps on the mean squared difference to the
        shape's distance at `batch` uniform points of [-1, 1]^3.  Nothing without a shape_init."""
        if self.shape_init is None:
            if self.force_shape_init:
                raise ValueError("ImplicitSDF: force_shape_init needs a shape_init")
            return
        if self.shape_init == "ellipsoid":
            if not (hasattr(self.shape_init_params, "__len__") and len(self.shape_init_params) == 3):
                raise ValueError("ImplicitSDF: shape_init 'ellipsoid' needs three semi-axes in shape_init_params")
            size = torch.as_tensor(self.shape_init_params, dtype=torch.float32, device=self.bbox.device)

            def truth(p):
                return ((p / size) ** 2).sum(dim=-1, keepdim=True).sqrt() - 1.0
        elif self.shape_init == "sphere":
            if not _is_number(self.shape_init_params):
                raise ValueError("ImplicitSDF: shape_init 'sphere' needs a radius in shape_init_params")
            radius = float(self.shape_init_params)

            def truth(p):
                return (p ** 2).sum(dim=-1, keepdim=True).sqrt() - radius
        elif self.shape_init.startswith("mesh:"):
            raise NotImplementedError("ImplicitSDF: shape_init 'mesh:' needs trimesh and pysdf, which this project does not depend on")
        else:
            raise ValueError("ImplicitSDF: unknown shape initialization type: %s" % self.shape_init)
        optim = torch.optim.Adam(self.parameters(), lr=lr)
        with torch.enable_grad():
            for _ in range(int(steps)):
                points = torch.rand((int(batch), 3), dtype=torch.float32, device=self.bbox.device) * 2.0 - 1.0
                loss = nn.functional.mse_loss(self.forward_sdf(points), truth(points))
                optim.zero_grad()
                loss.backward()
                optim.step()

    def isosurface(self, resolution=64, tets_path=None, threshold=0.0, chunk=1 << 20):
        """The Mesh (utils.mesh_geometry.Mesh) of sdf == threshold, extracted by marching tetrahedra on the grid of
        MarchingTetrahedraHelper(resolution, tets_path) laid over the box: where the NeuS stage hands over to the tetrahedral one.
        The vertices are in world coordinates and differentiable in the field's parameters."""
        from .isosurface import MarchingTetrahedraHelper, scale_tensor
        key = (int(resolution), tets_path)
        if key not in self._helpers:
            self._helpers[key] = MarchingTetrahedraHelper(*key)
        helper = self._helpers[key].to(self.bbox.device)
        points = scale_tensor(helper.grid_vertices, helper.points_range, self.bbox)
        level = self.forward_level(_chunked(self.forward_sdf, int(chunk), points), float(threshold))
        mesh = helper(level)
        mesh.v_pos = scale_tensor(mesh.v_pos, helper.points_range, self.bbox)
        return mesh


class NeuSVolumeRenderer(nn.Module):
    """The reference's neus-volume-renderer over a geometry with `bbox`, `radius`, forward and forward_sdf (ImplicitSDF): an
    OccupancyGrid of 32^3 cells, steps of 1.732 * 2 * radius / num_samples_per_ray, a LearnedVariance, the colour sigmoid(features)
    (the reference's no-material) and a solid background.  Materials with lights and the learned backgrounds are not offered.
    forward(rays_o [B, H, W, 3], rays_d, bg_color=None) returns comp_rgb, comp_rgb_fg, comp_rgb_bg [B, H, W, 3], opacity, depth
    [B, H, W, 1] and inv_std; in training also weights [M, 1], t_points, t_intervals [M, 1], t_dirs, points [M, 3], ray_indices [M] and
    the geometry's outputs; in eval comp_normal [B, H, W, 3].  bg_color: [3], [B, 3] or [B, H, W, 3]; black when absent.
    fused=True with NeuS alpha: one render_sdf_rays call a forward (one launch, and one in the backward), the normals riding as extra
    channels in eval.  fused=False or use_volsdf=True: neus_alpha / volsdf_density, render_weight_from_alpha and accumulate_along_rays.
    A batch without a single sample is the background, with zero gradients."""

    def __init__(self, geometry, num_samples_per_ray=512, randomized=True, eval_chunk_size=160000, grid_prune=True, prune_alpha_threshold=True,
                 learned_variance_init=0.3, cos_anneal_end_steps=0, use_volsdf=False, fused=True):
        super().__init__()
        if int(num_samples_per_ray) < 1:
            raise ValueError("NeuSVolumeRenderer: num_samples_per_ray must be at least 1")
        if int(cos_anneal_end_steps) < 0:
            raise ValueError("NeuSVolumeRenderer: cos_anneal_end_steps must not be negative")
        self.geometry = geometry
        self.num_samples_per_ray, self.grid_prune = int(num_samples_per_ray), bool(grid_prune)
        self.prune_alpha_threshold, self.eval_chunk_size = bool(prune_alpha_threshold), int(eval_chunk_size)
        self.cos_anneal_end_steps, self.use_volsdf, self.fused = int(cos_anneal_end_steps), bool(use_volsdf), bool(fused)
        self.cfg_randomized = bool(randomized)
        self.variance = LearnedVariance(learned_variance_init).to(geometry.bbox.device)
        self.estimator = OccupancyGrid(geometry.bbox.reshape(-1), resolution=32).to(geometry.bbox.device)
        if not self.grid_prune:
            self.estimator.occs.fill_(1.0)
            self.estimator.binaries.fill_(True)
        self.render_step_size = 1.732 * 2 * float(geometry.radius) / self.num_samples_per_ray
        self.cos_anneal_ratio = 1.0

    @property
    def randomized(self):
        return self.training and self.cfg_randomized

    def _step_alpha(self, sdf):
        """alpha of sdf [...] over one render step: the reference's alpha_fn and occ_eval_fn."""
        inv_std = self.variance(sdf)
        if self.use_volsdf:
            return self.render_step_size * volsdf_density(sdf, inv_std)
        return neus_alpha(sdf, None, None, self.render_step_size, inv_std)

    def forward(self, rays_o, rays_d, bg_color=None):
        if not (isinstance(rays_o, torch.Tensor) and rays_o.dim() == 4 and rays_o.shape[-1] == 3 and isinstance(rays_d, torch.Tensor) and
                rays_d.shape == rays_o.shape):
            raise ValueError("NeuSVolumeRenderer: rays_o and rays_d must be [B, H, W, 3]")
        B, H, W = rays_o.shape[:3]
        o, d = rays_o.reshape(-1, 3).contiguous(), rays_d.reshape(-1, 3).contiguous()
        n_rays = o.shape[0]
        geometry = self.geometry

        def alpha_fn(t_starts, t_ends, ray_indices):
            index = ray_indices.long()
            points = o[index] + d[index] * ((t_starts + t_ends) / 2.0)[:, None]
            if self.training:
                return self._step_alpha(geometry.forward_sdf(points)[..., 0])
            return self._step_alpha(_chunked(geometry.forward_sdf, self.eval_chunk_size, points)[..., 0])

        prune = self.grid_prune and self.prune_alpha_threshold
        ray_indices, t_starts, t_ends = self.estimator.sampling(
            o, d, alpha_fn=alpha_fn if prune else None, render_step_size=self.render_step_size, alpha_thre=0.01 if prune else 0.0,
            stratified=self.randomized, early_stop_eps=1e-4 if self.grid_prune else 0.0, max_samples_per_ray=self.num_samples_per_ray + 1)
        index = ray_indices.long()
        t_dirs = d[index]
        t_positions = ((t_starts + t_ends) / 2.0)[:, None]
        positions = o[index] + t_dirs * t_positions
        if self.training:
            geo = geometry(positions, output_normal=True)
        else:
            geo = _chunked(geometry, self.eval_chunk_size, positions, output_normal=True)
        rgb = torch.sigmoid(geo["features"])
        C = rgb.shape[-1]
        sdf, normal = geo["sdf"][..., 0].contiguous(), geo["normal"].contiguous()
        with_normal = not self.training

        if self.fused and not self.use_volsdf:
            values = torch.cat((rgb, normal), dim=-1) if with_normal else rgb
            inv_std = self.variance.inv_std.clamp(1.0e-6, 1.0e6).reshape(1)
            out, weights, _ = render_sdf_rays(sdf, normal, d, t_starts, t_ends, values.contiguous(), inv_std, ray_indices, n_rays,
                                              self.cos_anneal_ratio)
            opacity, depth, comp_rgb_fg = out[:, 0:1], out[:, 1:2], out[:, 2:2 + C]
            comp_normal = out[:, 2 + C:] if with_normal else None
        else:
            t_intervals = t_ends - t_starts
            if self.use_volsdf:
                alpha = torch.abs(t_intervals.detach()) * volsdf_density(sdf, self.variance(sdf))
            else:
                alpha = neus_alpha(sdf, normal, t_dirs, t_intervals, self.variance(sdf), self.cos_anneal_ratio)
            weights, _ = render_weight_from_alpha(alpha.contiguous(), ray_indices, n_rays)
            opacity = accumulate_along_rays(weights, None, ray_indices, n_rays)
            depth = accumulate_along_rays(weights, t_positions, ray_indices, n_rays)
            comp_rgb_fg = accumulate_along_rays(weights, rgb.contiguous(), ray_indices, n_rays)
            comp_normal = accumulate_along_rays(weights, normal, ray_indices, n_rays) if with_normal else None

        bg = _background("NeuSVolumeRenderer", bg_color, B, H, W, C, o.device)
        comp_rgb = comp_rgb_fg + bg * (1.0 - opacity)
        out = {"comp_rgb": comp_rgb.view(B, H, W, -1), "comp_rgb_fg": comp_rgb_fg.reshape(B, H, W, -1), "comp_rgb_bg": bg.reshape(B, H, W, -1),
               "opacity": opacity.reshape(B, H, W, 1), "depth": depth.reshape(B, H, W, 1)}
        if self.training:
            out.update(weights=weights[:, None], t_points=t_positions, t_intervals=(t_ends - t_starts)[:, None], t_dirs=t_dirs,
                       ray_indices=index, points=positions, **geo)
        else:
            comp_normal = nn.functional.normalize(comp_normal, dim=-1)
            out["comp_normal"] = ((comp_normal + 1.0) / 2.0 * opacity).view(B, H, W, 3)
        out["inv_std"] = self.variance.inv_std
        return out

    def update_step(self, global_step):
        """The reference's update_step: cos_anneal_ratio = min(1, global_step / cos_anneal_end_steps) (1 without an end), the
        geometry's own update_step, and in training with grid_prune the occupancy grid learns the alpha of one render step every
        16th step."""
        self.cos_anneal_ratio = 1.0 if self.cos_anneal_end_steps == 0 else min(1.0, int(global_step) / self.cos_anneal_end_steps)
        if hasattr(self.geometry, "update_step"):
            self.geometry.update_step(int(global_step))
        if self.grid_prune and self.training:
            self.estimator.update_every_n_steps(step=int(global_step), occ_eval_fn=lambda x: self._step_alpha(self.geometry.forward_sdf(x)))
