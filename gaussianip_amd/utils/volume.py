"""Volume rendering of a density field (csrc/volume.hip, gip_volume_*): marching rays through an occupancy grid and compositing along
them with gradients, under the names and argument order of nerfacc as the reference's nerf-volume-renderer calls it
(threestudio/models/renderers/nerf_volume_renderer.py).  nerfacc is CUDA-only; the definition is the kernel file's header, the
project's own, and has not been compared with nerfacc's output.

  march_rays(rays_o, rays_d, occ, aabb, render_step_size, ...)    (ray_indices, t_starts, t_ends, offsets): the samples of every ray
  render_weight_from_density(t_starts, t_ends, sigmas, ...)       (weights, trans, alphas); gradient to sigmas.  First order only.
  accumulate_along_rays(weights, values, ray_indices, n_rays)     [n_rays, C]; gradients to weights and values.  First order only.
  OccupancyGrid                    stands in for nerfacc.OccGridEstimator(levels=1): update_every_n_steps, sampling (pruning by a
                                   sigma_fn, or by an alpha_fn for utils/sdf_volume.py's signed-distance fields)
  ImplicitVolume                   the reference's implicit-volume geometry over get_encoding / get_mlp
  NeRFVolumeRenderer               the reference's nerf-volume-renderer with the no-material and a solid background
  get_ray_directions, get_rays     the reference's threestudio/utils/ops.py:179-260 without the camera noise

Every kernel output is bitwise equal from run to run: nothing is summed with atomics.  There is no CPU path for the kernels: their
inputs are float32 GPU tensors, anything else raises ValueError.  OccupancyGrid.update_every_n_steps, the pruning mask, the density
bias and the ray helpers are plain PyTorch and run wherever their tensors live."""
import math

import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from .._lib import call_model, ptr
from .encoding import get_activation, get_encoding, get_mlp

__all__ = ["march_rays", "render_weight_from_density", "accumulate_along_rays", "OccupancyGrid", "ImplicitVolume", "NeRFVolumeRenderer",
           "get_ray_directions", "get_rays"]

MAX_GRID = 256
MAX_CHANNELS = 16
_INT32_MAX = 2 ** 31 - 1
_MAX_RAYS = _INT32_MAX // 64


def _is_f32_gpu(t, dim):
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == dim


def _box(aabb):
    """(lo, hi) of an aabb given as six numbers or as [2, 3], as float32 numpy arrays."""
    box = np.asarray(aabb.detach().cpu() if isinstance(aabb, torch.Tensor) else aabb, dtype=np.float32).reshape(-1)
    if box.shape != (6,) or not np.isfinite(box).all() or not (box[:3] < box[3:]).all():
        raise ValueError("aabb must be six finite numbers (lo, hi) with lo < hi on every axis")
    return box[:3], box[3:]


def march_rays(rays_o, rays_d, occ, aabb, render_step_size, near_plane=0.0, far_plane=1e10, jitter=None, max_samples_per_ray=1024):
    """The samples of rays marched through the occupied cells of a grid: (ray_indices [M] int32, t_starts [M], t_ends [M],
    offsets [R + 1] int32), a ray's samples adjacent and ordered by t, ray r's being the rows offsets[r] .. offsets[r + 1] - 1.
    rays_o, rays_d [R, 3] float32 GPU tensors; occ [G, G, G] bool or uint8 on the same device, indexed [ix, iy, iz] over the box aabb
    (six numbers lo, hi, or [2, 3]); candidates are render_step_size long, start at the later of near_plane and the box's entry
    (shifted by jitter [R] in [0, 1) steps when given) and end at the earlier of far_plane and the exit; at most max_samples_per_ray
    candidates a ray.  Two launches and one host read (the total) between them.  Not differentiable."""
    if not (_is_f32_gpu(rays_o, 2) and rays_o.shape[1] == 3 and _is_f32_gpu(rays_d, 2) and rays_d.shape == rays_o.shape and
            rays_d.device == rays_o.device):
        raise ValueError("march_rays: rays_o and rays_d must be [R, 3] float32 GPU tensors on one device")
    dev, R = rays_o.device, int(rays_o.shape[0])
    if not (isinstance(occ, torch.Tensor) and occ.device == dev and occ.dtype in (torch.bool, torch.uint8) and occ.dim() == 3 and
            occ.shape[0] == occ.shape[1] == occ.shape[2] and 1 <= occ.shape[0] <= MAX_GRID):
        raise ValueError("march_rays: occ must be a [G, G, G] bool or uint8 tensor on the rays' device, 1 <= G <= %d" % MAX_GRID)
    if jitter is not None and not (_is_f32_gpu(jitter, 1) and jitter.device == dev and jitter.shape[0] == R):
        raise ValueError("march_rays: jitter must be an [R] float32 GPU tensor on the rays' device")
    lo, hi = _box(aabb)
    dt, near, far, K_cap = float(render_step_size), float(near_plane), float(far_plane), int(max_samples_per_ray)
    if not (dt > 0 and math.isfinite(dt)) or math.isnan(near) or math.isnan(far) or K_cap < 1:
        raise ValueError("march_rays: render_step_size must be positive and finite, the planes numbers, max_samples_per_ray at least 1")
    if R > _MAX_RAYS or R * K_cap > _INT32_MAX:
        raise ValueError("march_rays: %d rays x %d samples do not fit 31 bits" % (R, K_cap))
    G = int(occ.shape[0])
    scale = np.float32(G) / (hi - lo)                                  # float32, on the host: the kernels and the tests read these bits
    grid = occ.detach().contiguous()
    grid = grid.view(torch.uint8) if grid.dtype == torch.bool else grid
    o, d = rays_o.detach().contiguous(), rays_d.detach().contiguous()
    jit = None if jitter is None else jitter.detach().contiguous()
    args = (ptr(o), ptr(d), ptr(grid), ptr(jit), R, G) + tuple(float(v) for v in (*lo, *hi, *scale)) + (dt, near, far, K_cap)
    with torch.cuda.device(dev):
        offsets = torch.zeros(R + 1, dtype=torch.int32, device=dev)
        M = 0
        if R:
            counts = torch.empty(R, dtype=torch.int32, device=dev)
            call_model(dev, "gip_volume_march_count", *args, ptr(counts))
            offsets[1:] = torch.cumsum(counts, 0)
            M = int(offsets[-1])                                         # the one host read
        ray_indices = torch.empty(M, dtype=torch.int32, device=dev)
        t_starts, t_ends = (torch.empty(M, dtype=torch.float32, device=dev) for _ in range(2))
        if M:
            call_model(dev, "gip_volume_march_emit", *args, ptr(offsets), M, ptr(ray_indices), ptr(t_starts), ptr(t_ends))
    return ray_indices, t_starts, t_ends, offsets


def _offsets(what, ray_indices, n_rays, M, dev):
    """(offsets [R + 1] int32, ray_indices [M] int32, R) from the sorted ray_indices: no host read, and monotone within [0, M]
    whatever the caller passed.  ray_indices None: one ray that holds every sample."""
    if ray_indices is None:
        if n_rays not in (None, 1):
            raise ValueError("%s: n_rays without ray_indices can only be 1" % what)
        return torch.tensor([0, M], dtype=torch.int32, device=dev), torch.zeros(M, dtype=torch.int32, device=dev), 1
    if not (isinstance(ray_indices, torch.Tensor) and ray_indices.device == dev and ray_indices.dtype in (torch.int32, torch.int64) and
            ray_indices.dim() == 1 and ray_indices.shape[0] == M):
        raise ValueError("%s: ray_indices must be an [M] int32 or int64 tensor on the samples' device" % what)
    if n_rays is None or not 0 <= int(n_rays) <= _MAX_RAYS:
        raise ValueError("%s: n_rays must be given with ray_indices, 0 .. %d" % (what, _MAX_RAYS))
    R = int(n_rays)
    idx = ray_indices.detach().contiguous()
    bounds = torch.arange(R + 1, dtype=idx.dtype, device=dev)
    return torch.searchsorted(idx, bounds).to(torch.int32), idx.to(torch.int32), R


class _Weights(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t_starts, t_ends, sigmas, offsets, R):
        dev, M = sigmas.device, int(sigmas.shape[0])
        ts, te, sg = t_starts.detach().contiguous(), t_ends.detach().contiguous(), sigmas.detach().contiguous()
        with torch.cuda.device(dev):
            weights, trans, alphas = (torch.zeros(M, dtype=torch.float32, device=dev) for _ in range(3))
            if M and R:
                call_model(dev, "gip_volume_weights_forward", ptr(ts), ptr(te), ptr(sg), ptr(offsets), R, M, ptr(weights), ptr(trans),
                           ptr(alphas))
        ctx.save_for_backward(ts, te, weights, trans, alphas, offsets)
        ctx.R = R
        ctx.mark_non_differentiable(trans, alphas)
        return weights, trans, alphas

    @staticmethod
    @once_differentiable
    def backward(ctx, g_weights, _g_trans, _g_alphas):
        ts, te, weights, trans, alphas, offsets = ctx.saved_tensors
        dev, M = ts.device, int(ts.shape[0])
        g = g_weights.contiguous().float()
        with torch.cuda.device(dev):
            g_sigmas = torch.zeros(M, dtype=torch.float32, device=dev)
            if M and ctx.R:
                call_model(dev, "gip_volume_weights_backward", ptr(ts), ptr(te), ptr(g), ptr(weights), ptr(trans), ptr(alphas), ptr(offsets),
                           ctx.R, M, ptr(g_sigmas))
        return None, None, g_sigmas, None, None


def render_weight_from_density(t_starts, t_ends, sigmas, ray_indices=None, n_rays=None):
    """(weights, trans, alphas) [M] of the densities sigmas [M] on the samples (t_starts, t_ends) [M]: alpha = 1 - exp(-sigma (te - ts)),
    trans = exp(-the sum of sigma (te - ts) over the ray's earlier samples), weight = trans alpha.  ray_indices [M] (sorted, as
    march_rays returns them) with n_rays, or neither for one ray.  Differentiable in sigmas, first order only; trans and alphas carry no
    gradient, and the samples none either (they are drawn under no_grad).  Bitwise reproducible, forward and backward."""
    if not (_is_f32_gpu(sigmas, 1) and _is_f32_gpu(t_starts, 1) and _is_f32_gpu(t_ends, 1) and t_starts.shape == t_ends.shape == sigmas.shape and
            t_starts.device == t_ends.device == sigmas.device):
        raise ValueError("render_weight_from_density: t_starts, t_ends and sigmas must be [M] float32 GPU tensors on one device")
    offsets, _, R = _offsets("render_weight_from_density", ray_indices, n_rays, int(sigmas.shape[0]), sigmas.device)
    return _Weights.apply(t_starts, t_ends, sigmas, offsets, R)


_kernel_weights = render_weight_from_density          # what OccupancyGrid.sampling prunes by, whatever the public name is bound to


class _Accumulate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, values, offsets, ray_indices, R):
        dev, M = weights.device, int(weights.shape[0])
        C = 1 if values is None else int(values.shape[1])
        w = weights.detach().contiguous()
        v = None if values is None else values.detach().contiguous()
        with torch.cuda.device(dev):
            out = torch.zeros((R, C), dtype=torch.float32, device=dev)
            if M and R:
                call_model(dev, "gip_volume_accumulate_forward", ptr(w), ptr(v), ptr(offsets), R, M, C, ptr(out))
        ctx.save_for_backward(w, v, ray_indices)
        ctx.R, ctx.C = R, C
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        w, v, ray_indices = ctx.saved_tensors
        dev, M, R, C = w.device, int(w.shape[0]), ctx.R, ctx.C
        g = g_out.contiguous().float()
        need_w, need_v = ctx.needs_input_grad[0], v is not None and ctx.needs_input_grad[1]
        g_w = g_v = None
        with torch.cuda.device(dev):
            if need_w:
                g_w = torch.zeros(M, dtype=torch.float32, device=dev)
            if need_v:
                g_v = torch.zeros((M, C), dtype=torch.float32, device=dev)
            if M and R and (need_w or need_v):
                call_model(dev, "gip_volume_accumulate_backward", ptr(w), ptr(v), ptr(ray_indices), ptr(g), R, M, C, ptr(g_w), ptr(g_v))
        return g_w, g_v, None, None, None


def accumulate_along_rays(weights, values=None, ray_indices=None, n_rays=None):
    """out [n_rays, C]: the sum over every ray's samples of weights [M] x values [M, C], C = 1 .. 16; values None counts as ones, C = 1.
    Rays without samples give 0.  ray_indices [M] (sorted) with n_rays, or neither for one ray.  Differentiable in weights and values,
    first order only.  A segmented sum in a fixed order, without atomics: bitwise reproducible, forward and backward."""
    if not _is_f32_gpu(weights, 1):
        raise ValueError("accumulate_along_rays: weights must be an [M] float32 GPU tensor")
    M = int(weights.shape[0])
    if values is not None and not (_is_f32_gpu(values, 2) and values.device == weights.device and values.shape[0] == M and
                                   1 <= values.shape[1] <= MAX_CHANNELS):
        raise ValueError("accumulate_along_rays: values must be an [M, C] float32 GPU tensor on the weights' device, C = 1 .. %d" % MAX_CHANNELS)
    if M * (1 if values is None else int(values.shape[1])) > _INT32_MAX:
        raise ValueError("accumulate_along_rays: %d samples x channels do not fit 31 bits" % M)
    offsets, idx, R = _offsets("accumulate_along_rays", ray_indices, n_rays, M, weights.device)
    return _Accumulate.apply(weights, values, offsets, idx, R)


def prune_mask(trans, alphas, alpha_thre, early_stop_eps):
    """The samples OccupancyGrid.sampling keeps: alphas >= alpha_thre and trans >= early_stop_eps."""
    return (alphas >= alpha_thre) & (trans >= early_stop_eps)


class OccupancyGrid(nn.Module):
    """Stands in for nerfacc.OccGridEstimator(roi_aabb=aabb, resolution=resolution, levels=1): a resolution^3 grid over the box aabb
    with the buffers occs [G^3] (float, a decayed maximum of what occ_eval_fn returned) and binaries [G, G, G] (bool, indexed
    [ix, iy, iz]; what the march reads).  Both start empty, as nerfacc's do."""

    def __init__(self, aabb, resolution=32):
        super().__init__()
        G = int(resolution)
        if not 1 <= G <= MAX_GRID:
            raise ValueError("OccupancyGrid: resolution must lie in 1 .. %d" % MAX_GRID)
        lo, hi = _box(aabb)
        self.resolution = G
        self._lo_hi = (lo, hi)                                           # the host's copy: a march reads no device value for its box
        self.register_buffer("aabb", torch.from_numpy(np.concatenate((lo, hi))))
        self.register_buffer("occs", torch.zeros(G ** 3, dtype=torch.float32))
        self.register_buffer("binaries", torch.zeros((G, G, G), dtype=torch.bool))

    @torch.no_grad()
    def update_every_n_steps(self, step, occ_eval_fn, occ_thre=0.01, ema_decay=0.95, warmup_steps=256, n=16):
        """Every n-th step: occ_eval_fn at one uniformly random point of every chosen cell ([N, 3] -> [N] or [N, 1]); all cells while
        step < warmup_steps, afterwards a uniformly random quarter plus the occupied ones; occs = max(occs * ema_decay, occ) there;
        binaries = occs > min(occs.mean(), occ_thre).  Plain PyTorch on G^3 cells."""
        if int(step) % int(n) != 0:
            return
        G, dev = self.resolution, self.occs.device
        cells = G ** 3
        if step < warmup_steps:
            chosen = torch.arange(cells, device=dev)
        else:
            uniform = torch.randint(cells, (cells // 4,), device=dev)
            chosen = torch.unique(torch.cat((uniform, torch.nonzero(self.binaries.reshape(-1))[:, 0])))
        coords = torch.stack((chosen // (G * G), chosen // G % G, chosen % G), dim=-1).float()
        lo, hi = self.aabb[:3], self.aabb[3:]
        x = lo + (coords + torch.rand_like(coords)) / G * (hi - lo)
        occ = occ_eval_fn(x).reshape(-1).float()
        self.occs[chosen] = torch.maximum(self.occs[chosen] * ema_decay, occ)
        threshold = torch.clamp(self.occs.mean(), max=occ_thre)
        self.binaries.copy_((self.occs > threshold).view(G, G, G))

    @torch.no_grad()
    def sampling(self, rays_o, rays_d, sigma_fn=None, render_step_size=1e-3, alpha_thre=0.0, stratified=False, early_stop_eps=1e-4,
                 near_plane=0.0, far_plane=1e10, max_samples_per_ray=1024, alpha_fn=None):
        """(ray_indices, t_starts, t_ends) of march_rays through binaries; stratified draws jitter = torch.rand(R).  With sigma_fn
        (t_starts, t_ends, ray_indices -> sigmas [M]) and alpha_thre > 0 or early_stop_eps > 0, only the samples with
        alphas >= alpha_thre and trans >= early_stop_eps are kept, trans and alphas being render_weight_from_density's on the marched
        samples; the mask and the compaction are PyTorch.  With alpha_fn (the same arguments -> alphas [M]) instead, the alphas are
        the given ones and trans is utils.sdf_volume.render_weight_from_alpha's.  Both functions together: ValueError."""
        if sigma_fn is not None and alpha_fn is not None:
            raise ValueError("OccupancyGrid.sampling: give sigma_fn or alpha_fn, not both")
        jitter = torch.rand(rays_o.shape[0], device=rays_o.device) if stratified and isinstance(rays_o, torch.Tensor) else None
        ray_indices, t_starts, t_ends, _ = march_rays(rays_o, rays_d, self.binaries, self._lo_hi, render_step_size, near_plane, far_plane,
                                                      jitter, max_samples_per_ray)
        if sigma_fn is not None and (alpha_thre > 0 or early_stop_eps > 0) and ray_indices.shape[0]:
            sigmas = sigma_fn(t_starts, t_ends, ray_indices).reshape(-1).float().contiguous()
            _, trans, alphas = _kernel_weights(t_starts, t_ends, sigmas, ray_indices, int(rays_o.shape[0]))
            keep = prune_mask(trans, alphas, alpha_thre, early_stop_eps)
            ray_indices, t_starts, t_ends = ray_indices[keep], t_starts[keep], t_ends[keep]
        elif alpha_fn is not None and (alpha_thre > 0 or early_stop_eps > 0) and ray_indices.shape[0]:
            from .sdf_volume import render_weight_from_alpha
            alphas = alpha_fn(t_starts, t_ends, ray_indices).reshape(-1).float().contiguous()
            _, trans = render_weight_from_alpha(alphas, ray_indices, int(rays_o.shape[0]))
            keep = prune_mask(trans, alphas, alpha_thre, early_stop_eps)
            ray_indices, t_starts, t_ends = ray_indices[keep], t_starts[keep], t_ends[keep]
        return ray_indices, t_starts, t_ends


DENSITY_ACTIVATIONS = ("softplus", "exp", "relu", "none")
NORMAL_TYPES = (None, "finite_difference", "finite_difference_laplacian", "pred")


class ImplicitVolume(nn.Module):
    """The reference's implicit-volume geometry (threestudio/models/geometry/implicit_volume.py:58-230): a position encoding over the
    box [-radius, radius]^3 with one MLP for the density and one for n_feature_dims features.  The configuration keys are keyword
    arguments; the encoding and MLP configurations default to the reference's (a 16-level hash grid, one hidden layer of 64).
    density = activation(network + bias), bias = density_blob_scale * (1 - |x| / density_blob_std) for "blob_magic3d",
    density_blob_scale * exp(-|x|^2 / (2 density_blob_std^2)) for "blob_dreamfusion", or a number.  normal_type "analytic" needs second
    derivatives of the encoding, which is first order only: ValueError."""

    def __init__(self, radius=1.0, n_feature_dims=3, density_activation="softplus", density_bias="blob_magic3d", density_blob_scale=10.0,
                 density_blob_std=0.5, pos_encoding_config=None, mlp_network_config=None, normal_type="finite_difference",
                 finite_difference_normal_eps=0.01):
        super().__init__()
        if not float(radius) > 0:
            raise ValueError("ImplicitVolume: radius must be positive")
        key = "none" if density_activation is None else str(density_activation).lower()
        if key not in DENSITY_ACTIVATIONS:
            raise ValueError("ImplicitVolume: density_activation must be one of %s" % (DENSITY_ACTIVATIONS,))
        if not (density_bias in ("blob_magic3d", "blob_dreamfusion") or (isinstance(density_bias, (int, float)) and not isinstance(density_bias, bool))):
            raise ValueError("ImplicitVolume: unknown density bias %r" % (density_bias,))
        if normal_type not in NORMAL_TYPES:
            raise ValueError("ImplicitVolume: normal_type must be one of %s (the hash grid is first order only: no \"analytic\")" % (NORMAL_TYPES,))
        self.radius, self.n_feature_dims = float(radius), int(n_feature_dims)
        self.density_activation, self.density_bias = key, density_bias
        self.density_blob_scale, self.density_blob_std = float(density_blob_scale), float(density_blob_std)
        self.normal_type, self.finite_difference_normal_eps = normal_type, float(finite_difference_normal_eps)
        self.register_buffer("bbox", torch.tensor([[-self.radius] * 3, [self.radius] * 3], dtype=torch.float32))
        encoding = dict(pos_encoding_config or {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19,
                                                "base_resolution": 16, "per_level_scale": 1.447269237440378})
        mlp = dict(mlp_network_config or {"otype": "VanillaMLP", "activation": "ReLU", "output_activation": "none", "n_neurons": 64,
                                          "n_hidden_layers": 1})
        self.encoding = get_encoding(3, encoding)
        self.density_network = get_mlp(self.encoding.n_output_dims, 1, mlp)
        if self.n_feature_dims > 0:
            self.feature_network = get_mlp(self.encoding.n_output_dims, self.n_feature_dims, mlp)
        if normal_type == "pred":
            self.normal_network = get_mlp(self.encoding.n_output_dims, 3, mlp)

    def get_activated_density(self, points, density):
        """(raw, activated) density [..., 1] of the network's output `density` [..., 1] at `points` [..., 3] (world coordinates)."""
        if self.density_bias == "blob_dreamfusion":
            bias = self.density_blob_scale * torch.exp(-0.5 * (points ** 2).sum(dim=-1) / self.density_blob_std ** 2)[..., None]
        elif self.density_bias == "blob_magic3d":
            bias = self.density_blob_scale * (1 - torch.sqrt((points ** 2).sum(dim=-1)) / self.density_blob_std)[..., None]
        else:
            bias = float(self.density_bias)
        raw = density + bias
        return raw, get_activation(self.density_activation)(raw)

    def _unit(self, points):
        """The box mapped to [0, 1]^3: the reference's contract_to_unisphere(..., unbounded=False)."""
        return (points - self.bbox[0]) / (self.bbox[1] - self.bbox[0])

    def forward_density(self, points):
        """density [..., 1] at points [..., 3]."""
        net = self.density_network(self.encoding(self._unit(points).reshape(-1, 3))).reshape(*points.shape[:-1], 1)
        return self.get_activated_density(points, net)[1]

    def forward(self, points, output_normal=False):
        """{"density" [..., 1], "features" [..., n_feature_dims] when there are any, and with output_normal "normal" and "shading_normal"
        [..., 3]} at points [..., 3]: the reference's dict."""
        enc = self.encoding(self._unit(points).reshape(-1, 3))
        density = self.get_activated_density(points, self.density_network(enc).view(*points.shape[:-1], 1))[1]
        out = {"density": density}
        if self.n_feature_dims > 0:
            out["features"] = self.feature_network(enc).view(*points.shape[:-1], self.n_feature_dims)
        if output_normal:
            eps = self.finite_difference_normal_eps
            if self.normal_type == "finite_difference_laplacian":
                shifts = torch.tensor([[eps, 0, 0], [-eps, 0, 0], [0, eps, 0], [0, -eps, 0], [0, 0, eps], [0, 0, -eps]]).to(points)
                moved = self.forward_density((points[..., None, :] + shifts).clamp(-self.radius, self.radius))
                normal = -0.5 * (moved[..., 0::2, 0] - moved[..., 1::2, 0]) / eps
            elif self.normal_type == "finite_difference":
                shifts = torch.tensor([[eps, 0, 0], [0, eps, 0], [0, 0, eps]]).to(points)
                moved = self.forward_density((points[..., None, :] + shifts).clamp(-self.radius, self.radius))
                normal = -(moved[..., 0] - density) / eps
            elif self.normal_type == "pred":
                normal = self.normal_network(enc).view(*points.shape[:-1], 3)
            else:
                raise ValueError("ImplicitVolume: output_normal needs a normal_type")
            normal = nn.functional.normalize(normal, dim=-1)
            out.update(normal=normal, shading_normal=normal)
        return out


def _chunked(fn, chunk, points, **kwargs):
    """fn(points, **kwargs) in chunks of `chunk` rows, the dicts' entries (or the tensors) joined: the reference's chunk_batch."""
    if chunk <= 0 or points.shape[0] <= chunk:
        return fn(points, **kwargs)
    parts = [fn(points[i:i + chunk], **kwargs) for i in range(0, points.shape[0], chunk)]
    if isinstance(parts[0], dict):
        return {k: torch.cat([p[k] for p in parts], dim=0) for k in parts[0]}
    return torch.cat(parts, dim=0)


def _background(what, bg_color, B, H, W, C, dev):
    """bg [B H W, C] of a renderer's bg_color: [C], [B, C] or [B, H, W, C]; black when absent."""
    n_rays = B * H * W
    if bg_color is None:
        return torch.zeros((n_rays, C), dtype=torch.float32, device=dev)
    bg = torch.as_tensor(bg_color, dtype=torch.float32, device=dev)
    if bg.dim() == 1:
        return bg.expand(n_rays, C)
    if tuple(bg.shape[:-1]) == (B,):
        return bg[:, None, None, :].expand(B, H, W, bg.shape[-1]).reshape(n_rays, -1)
    if tuple(bg.shape[:-1]) == (B, H, W):
        return bg.reshape(n_rays, -1)
    raise ValueError("%s: bg_color must be [3], [B, 3] or [B, H, W, 3]" % what)


class NeRFVolumeRenderer(nn.Module):
    """The reference's nerf-volume-renderer over a geometry with `bbox`, `radius`, forward and forward_density (ImplicitVolume): an
    OccupancyGrid of 32^3 cells, steps of 1.732 * 2 * radius / num_samples_per_ray, the colour sigmoid(features) (the reference's
    no-material) and a solid background.  Materials with lights and the learned backgrounds are not offered.
    forward(rays_o [B, H, W, 3], rays_d, bg_color=None) returns comp_rgb, comp_rgb_fg, comp_rgb_bg [B, H, W, 3], opacity, depth and
    z_variance [B, H, W, 1]; in training also weights [M, 1], t_points, t_intervals [M, 1], t_dirs, points [M, 3], ray_indices [M]
    and the geometry's outputs; comp_normal [B, H, W, 3] with return_comp_normal.  bg_color: [3], [B, 3] or [B, H, W, 3]; black when
    absent.  A batch without a single sample is the background, with zero gradients."""

    def __init__(self, geometry, num_samples_per_ray=512, randomized=True, grid_prune=True, prune_alpha_threshold=True, eval_chunk_size=160000,
                 return_comp_normal=False):
        super().__init__()
        if int(num_samples_per_ray) < 1:
            raise ValueError("NeRFVolumeRenderer: num_samples_per_ray must be at least 1")
        self.geometry = geometry
        self.num_samples_per_ray, self.grid_prune = int(num_samples_per_ray), bool(grid_prune)
        self.prune_alpha_threshold, self.eval_chunk_size = bool(prune_alpha_threshold), int(eval_chunk_size)
        self.return_comp_normal = bool(return_comp_normal)
        self.cfg_randomized = bool(randomized)
        self.estimator = OccupancyGrid(geometry.bbox.reshape(-1), resolution=32).to(geometry.bbox.device)
        if not self.grid_prune:
            self.estimator.occs.fill_(1.0)
            self.estimator.binaries.fill_(True)
        self.render_step_size = 1.732 * 2 * float(geometry.radius) / self.num_samples_per_ray

    @property
    def randomized(self):
        return self.training and self.cfg_randomized

    def forward(self, rays_o, rays_d, bg_color=None):
        if not (isinstance(rays_o, torch.Tensor) and rays_o.dim() == 4 and rays_o.shape[-1] == 3 and isinstance(rays_d, torch.Tensor) and
                rays_d.shape == rays_o.shape):
            raise ValueError("NeRFVolumeRenderer: rays_o and rays_d must be [B, H, W, 3]")
        B, H, W = rays_o.shape[:3]
        o, d = rays_o.reshape(-1, 3).contiguous(), rays_d.reshape(-1, 3).contiguous()
        n_rays = o.shape[0]
        geometry = self.geometry

        def positions_of(t_starts, t_ends, ray_indices):
            index = ray_indices.long()
            return o[index] + d[index] * ((t_starts + t_ends) / 2.0)[:, None]

        def sigma_fn(t_starts, t_ends, ray_indices):
            points = positions_of(t_starts, t_ends, ray_indices)
            if self.training:
                return geometry.forward_density(points)[..., 0]
            return _chunked(geometry.forward_density, self.eval_chunk_size, points)[..., 0]

        prune = self.grid_prune and self.prune_alpha_threshold
        ray_indices, t_starts, t_ends = self.estimator.sampling(
            o, d, sigma_fn=sigma_fn if prune else None, render_step_size=self.render_step_size, alpha_thre=0.01 if prune else 0.0,
            stratified=self.randomized, early_stop_eps=1e-4 if self.grid_prune else 0.0, max_samples_per_ray=self.num_samples_per_ray + 1)
        index = ray_indices.long()
        t_dirs = d[index]
        t_positions = ((t_starts + t_ends) / 2.0)[:, None]
        positions = o[index] + t_dirs * t_positions
        normals = self.return_comp_normal
        if self.training:
            geo = geometry(positions, output_normal=normals)
        else:
            geo = _chunked(geometry, self.eval_chunk_size, positions, output_normal=normals)
        rgb = torch.sigmoid(geo["features"])

        weights, _, _ = render_weight_from_density(t_starts, t_ends, geo["density"][..., 0].contiguous(), ray_indices, n_rays)
        opacity = accumulate_along_rays(weights, None, ray_indices, n_rays)
        depth = accumulate_along_rays(weights, t_positions, ray_indices, n_rays)
        comp_rgb_fg = accumulate_along_rays(weights, rgb.contiguous(), ray_indices, n_rays)
        # the second moment about the ray's own depth, not E[t^2] - depth^2, which cancels
        z_variance = accumulate_along_rays(weights, ((t_positions - depth[index]) ** 2).contiguous(), ray_indices, n_rays)

        bg = _background("NeRFVolumeRenderer", bg_color, B, H, W, comp_rgb_fg.shape[-1], o.device)
        comp_rgb = comp_rgb_fg + bg * (1.0 - opacity)
        out = {"comp_rgb": comp_rgb.view(B, H, W, -1), "comp_rgb_fg": comp_rgb_fg.view(B, H, W, -1), "comp_rgb_bg": bg.reshape(B, H, W, -1),
               "opacity": opacity.view(B, H, W, 1), "depth": depth.view(B, H, W, 1), "z_variance": z_variance.view(B, H, W, 1)}
        if self.training:
            out.update(weights=weights[:, None], t_points=t_positions, t_intervals=(t_ends - t_starts)[:, None], t_dirs=t_dirs,
                       ray_indices=index, points=positions, **geo)
        if "normal" in geo:
            comp_normal = nn.functional.normalize(accumulate_along_rays(weights, geo["normal"].contiguous(), ray_indices, n_rays), dim=-1)
            out["comp_normal"] = ((comp_normal + 1.0) / 2.0 * opacity).view(B, H, W, 3)
        return out

    def update_step(self, global_step):
        """The reference's update_step: in training with grid_prune, the occupancy grid learns density * render_step_size (the first
        term of 1 - exp(-density * render_step_size)) every 16th step."""
        if self.grid_prune and self.training:
            self.estimator.update_every_n_steps(step=int(global_step), occ_eval_fn=lambda x: self.geometry.forward_density(x) * self.render_step_size)


def get_ray_directions(H, W, focal, principal=None, use_pixel_centers=True):
    """directions [H, W, 3] of the pixels' rays in camera coordinates (x right, y up, looking along -z), not normalised:
    ((i - cx) / fx, -(j - cy) / fy, -1) for column i and row j, at pixel centres unless use_pixel_centers is False.  focal: one number
    (then the principal point is the image centre) or (fx, fy) with principal = (cx, cy)."""
    if isinstance(focal, (int, float)):
        fx = fy = float(focal)
        cx, cy = W / 2, H / 2
    else:
        fx, fy = focal
        if principal is None:
            raise ValueError("get_ray_directions: (fx, fy) needs principal = (cx, cy)")
        cx, cy = principal
    shift = 0.5 if use_pixel_centers else 0.0
    j, i = torch.meshgrid(torch.arange(H, dtype=torch.float32) + shift, torch.arange(W, dtype=torch.float32) + shift, indexing="ij")
    return torch.stack(((i - cx) / fx, -(j - cy) / fy, -torch.ones_like(i)), dim=-1)


def get_rays(directions, c2w, keepdim=False):
    """(rays_o, rays_d) in world coordinates of directions [..., 3] under camera-to-world matrices c2w: [4, 4], or [B, 4, 4] for
    directions [H, W, 3] (one image per camera), [B, H, W, 3] or [N, 3] (one matrix per row, or one for all).  rays_d is normalised;
    both are flattened to [N, 3] unless keepdim."""
    if directions.shape[-1] != 3 or tuple(c2w.shape[-2:]) != (4, 4) or c2w.dim() not in (2, 3):
        raise ValueError("get_rays: directions [..., 3] and c2w [4, 4] or [B, 4, 4]")
    rot, origin = c2w[..., :3, :3], c2w[..., :3, 3]
    if c2w.dim() == 3 and directions.dim() == 3:
        directions = directions[None]
    if c2w.dim() == 3:
        lead = (c2w.shape[0],) + (1,) * (directions.dim() - 2)
        rot, origin = rot.reshape(lead + (3, 3)), origin.reshape(lead + (3,))
    rays_d = (directions[..., None, :] * rot).sum(-1)
    rays_o = origin.expand(rays_d.shape)
    rays_d = nn.functional.normalize(rays_d, dim=-1)
    if not keepdim:
        rays_o, rays_d = rays_o.reshape(-1, 3), rays_d.reshape(-1, 3)
    return rays_o, rays_d
