"""Position encodings and the small MLP behind them (csrc/hashgrid.hip, gip_hashgrid_*): the surface of the reference's
threestudio/models/networks.py by the same names, with the multiresolution hash grid that the reference takes from tinycudann written
for gfx950.  tinycudann is CUDA-only; the definition is the published Instant-NGP scheme as the kernel file's header states it, and the
table layout has not been checked against a tinycudann checkpoint.

  HashGridLayout(config)            the level table (scale, resolution, rows, offset and dense / hashed per level), n_params, n_output_dims
  hash_grid_encode(x, table, layout)  enc [N, L F] of x [N, 3]; gradients to table and, when x requires one, to x.  First order only.
  HashGridEncoding                  stands in for TCNNEncoding with otype HashGrid: the parameter `params` [P F], uniform in +-1e-4
  ProgressiveBandHashGrid, ProgressiveBandFrequency, CompositeEncoding, VanillaMLP, get_encoding, get_mlp: the reference's

The forward and the gradient to x are bitwise equal from run to run.  The gradient to the table is a scatter of float atomic adds and is
NOT: colliding rows are summed in the order the adds arrive.  There is no CPU path for the kernels: x and the table are float32 GPU
tensors, anything else raises ValueError.  The MLP is nn.Linear, that is the BLAS library's GEMM, in float32."""
import ctypes
import math

import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from .._lib import call_model, ptr

__all__ = ["HashGridLayout", "hash_grid_encode", "HashGridEncoding", "ProgressiveBandHashGrid", "ProgressiveBandFrequency",
           "CompositeEncoding", "VanillaMLP", "get_encoding", "get_mlp", "get_activation"]

MAX_LEVELS = 32
MAX_LOG2_HASHMAP_SIZE = 24
FEATURES_PER_LEVEL = (1, 2, 4, 8)
ENCODING_OTYPES = ("HashGrid", "ProgressiveBandHashGrid", "ProgressiveBandFrequency")
MLP_OTYPES = ("VanillaMLP",)
_UINT32_MAX = 2 ** 32 - 1


class HashGridLayout:
    """The level table of a hash grid, computed once from the configuration (a dict with n_levels, n_features_per_level,
    log2_hashmap_size, base_resolution, per_level_scale) and read by the kernels and by every restatement of them:
      scales [L] float32    exp2f(l * log2f(per_level_scale)) * base_resolution - 1, every step rounded to float32
      resolutions [L]       ceil(scale) + 1
      sizes [L]             min(round_up(resolution^3, 8), 2^log2_hashmap_size) rows
      offsets [L] int64     the running sum of the sizes
      hashed [L]            resolution^3 > size: the level's rows are hashed, else dense
    n_params = sum(sizes) * n_features_per_level, n_rows = sum(sizes), n_output_dims = n_levels * n_features_per_level.  Python
    integers do not overflow, so a cube above 2^log2_hashmap_size simply is too large.  Raises ValueError outside the limits."""

    def __init__(self, config):
        try:
            L, F = int(config["n_levels"]), int(config["n_features_per_level"])
            log2_size, base = int(config["log2_hashmap_size"]), config["base_resolution"]
            per_level_scale = float(config["per_level_scale"])
        except KeyError as exc:
            raise ValueError("hash grid configuration: missing %s" % exc) from None
        if config.get("interpolation", "Linear") != "Linear":
            raise ValueError("hash grid configuration: only Linear interpolation is offered")
        if not 1 <= L <= MAX_LEVELS:
            raise ValueError("n_levels must lie in 1 .. %d" % MAX_LEVELS)
        if F not in FEATURES_PER_LEVEL:
            raise ValueError("n_features_per_level must be one of %s" % (FEATURES_PER_LEVEL,))
        if not 0 <= log2_size <= MAX_LOG2_HASHMAP_SIZE:
            raise ValueError("log2_hashmap_size must lie in 0 .. %d" % MAX_LOG2_HASHMAP_SIZE)
        if not (float(base) >= 1 and math.isfinite(per_level_scale) and per_level_scale > 0):
            raise ValueError("base_resolution must be at least 1 and per_level_scale positive")
        self.n_levels, self.n_features_per_level, self.log2_hashmap_size = L, F, log2_size
        self.base_resolution, self.per_level_scale = base, per_level_scale
        level = np.arange(L, dtype=np.float32)
        with np.errstate(over="ignore"):
            self.scales = (np.exp2(level * np.log2(np.float32(per_level_scale))) * np.float32(base) - np.float32(1)).astype(np.float32)
        if not (np.isfinite(self.scales).all() and self.scales.min() >= 0 and self.scales.max() < 2.0 ** 30):
            raise ValueError("hash grid configuration: a level's scale is outside [0, 2^30)")
        cap = 1 << log2_size
        self.resolutions = [int(math.ceil(float(s))) + 1 for s in self.scales]
        self.sizes = [min((r ** 3 + 7) // 8 * 8, cap) for r in self.resolutions]
        self.hashed = [r ** 3 > t for r, t in zip(self.resolutions, self.sizes)]
        self.offsets = [sum(self.sizes[:l]) for l in range(L)]
        self.n_rows = sum(self.sizes)
        self.n_params = self.n_rows * F
        self.n_output_dims = L * F
        # what the entry points read: host arrays, kept alive with the layout
        self._arrays = (np.ascontiguousarray(self.scales), np.asarray(self.resolutions, np.int32), np.asarray(self.sizes, np.int32),
                        np.asarray(self.offsets, np.int64), np.asarray(self.hashed, np.int32))

    def level_args(self, N):
        """The entry points' arguments from the level table to P: five host arrays, then N, L, F, P."""
        return tuple(ctypes.c_void_p(a.ctypes.data) for a in self._arrays) + (int(N), self.n_levels, self.n_features_per_level, self.n_rows)

    def __repr__(self):
        return "HashGridLayout(L=%d, F=%d, rows=%d, %d dense + %d hashed levels)" % (
            self.n_levels, self.n_features_per_level, self.n_rows, self.hashed.count(False), self.hashed.count(True))


def _aligned(t):
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


class _HashGridEncode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, table, layout):
        dev = x.device
        xd, td = x.detach().contiguous(), _aligned(table.detach().contiguous())
        N = int(xd.shape[0])
        with torch.cuda.device(dev):
            enc = torch.empty((N, layout.n_output_dims), dtype=torch.float32, device=dev)
            if N:
                call_model(dev, "gip_hashgrid_forward", ptr(xd), ptr(td), *layout.level_args(N), ptr(enc))
        ctx.save_for_backward(xd, td)
        ctx.layout = layout
        return enc

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        xd, td = ctx.saved_tensors
        layout, dev, N = ctx.layout, xd.device, int(xd.shape[0])
        g = _aligned(g.contiguous().float())
        g_x = g_table = None
        with torch.cuda.device(dev):
            if ctx.needs_input_grad[0]:
                g_x = torch.zeros((N, 3), dtype=torch.float32, device=dev)
                if N:
                    call_model(dev, "gip_hashgrid_backward_input", ptr(xd), ptr(td), ptr(g), *layout.level_args(N), ptr(g_x))
            if ctx.needs_input_grad[1]:
                g_table = torch.zeros_like(td)                       # the scatter adds into zeros
                if N:
                    call_model(dev, "gip_hashgrid_backward_table", ptr(xd), ptr(g), *layout.level_args(N), ptr(g_table))
        return g_x, g_table, None


def hash_grid_encode(x, table, layout):
    """enc [N, L F] float32, level-major: the multiresolution hash-grid encoding of x [N, 3] (meant to lie in [0, 1]; anything else
    wraps around the level's slice, and a non-finite or huge coordinate gives zeros) with table [P, F], P = layout.n_rows.
    Differentiable in table and in x, first order only.  enc and the gradient to x are bitwise reproducible; the gradient to table is
    summed with float atomics and is not.  x and table must be float32 GPU tensors on one device; N F L 4 must fit 32 bits."""
    if not isinstance(layout, HashGridLayout):
        raise ValueError("hash_grid_encode: layout must be a HashGridLayout")
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == 3):
        raise ValueError("hash_grid_encode: x must be an [N, 3] float32 GPU tensor (three input dimensions only)")
    if not (isinstance(table, torch.Tensor) and table.is_cuda and table.dtype == torch.float32 and table.device == x.device and
            tuple(table.shape) == (layout.n_rows, layout.n_features_per_level)):
        raise ValueError("hash_grid_encode: table must be a [%d, %d] float32 GPU tensor on x's device" % (
            layout.n_rows, layout.n_features_per_level))
    if 4 * int(x.shape[0]) * layout.n_output_dims > _UINT32_MAX:
        raise ValueError("hash_grid_encode: %d points x %d outputs x 4 bytes does not fit 32 bits" % (x.shape[0], layout.n_output_dims))
    return _HashGridEncode.apply(x, table, layout)


def _grid_config(in_channels, config):
    if int(in_channels) != 3:
        raise ValueError("the hash grid encodes three input dimensions only, not %s" % (in_channels,))
    if not isinstance(config, dict):
        raise ValueError("the encoding's configuration must be a dict")
    return HashGridLayout(config)


class HashGridEncoding(nn.Module):
    """The reference's TCNNEncoding for otype HashGrid (or Grid with type Hash): forward(x [..., 3] in [0, 1]) -> [N, n_output_dims]
    with N the number of points.  `params` [n_params] float32 is the table, level after level, a row's features adjacent; it starts
    uniform in +-1e-4 as tinycudann's does.  n_input_dims and n_output_dims as in the reference."""

    def __init__(self, in_channels, config, dtype=torch.float32):
        super().__init__()
        if dtype != torch.float32:
            raise ValueError("HashGridEncoding: float32 only")
        self.layout = _grid_config(in_channels, config)
        self.n_input_dims, self.n_output_dims = 3, self.layout.n_output_dims
        self.params = nn.Parameter(torch.empty(self.layout.n_params, dtype=torch.float32).uniform_(-1e-4, 1e-4))

    def forward(self, x):
        return hash_grid_encode(x.reshape(-1, 3), self.params.view(self.layout.n_rows, self.layout.n_features_per_level), self.layout)


class ProgressiveBandHashGrid(nn.Module):
    """The reference's ProgressiveBandHashGrid: the hash grid times a mask over its outputs that opens level by level.  The mask
    starts at zero (as the reference's: nothing passes before the first update_step) and update_step(epoch, global_step) sets its
    first min(start_level + max(global_step - start_step, 0) // update_steps, n_levels) * n_features_per_level entries to 1."""

    def __init__(self, in_channels, config, dtype=torch.float32):
        super().__init__()
        for key in ("start_level", "start_step", "update_steps"):
            if key not in config:
                raise ValueError("ProgressiveBandHashGrid configuration: missing %r" % key)
        self.encoding = HashGridEncoding(in_channels, config, dtype)
        self.n_input_dims, self.n_output_dims = 3, self.encoding.n_output_dims
        self.n_level, self.n_features_per_level = int(config["n_levels"]), int(config["n_features_per_level"])
        self.start_level, self.start_step, self.update_steps = int(config["start_level"]), int(config["start_step"]), int(config["update_steps"])
        if self.update_steps < 1:
            raise ValueError("ProgressiveBandHashGrid configuration: update_steps must be at least 1")
        self.current_level = self.start_level
        self.register_buffer("mask", torch.zeros(self.n_level * self.n_features_per_level, dtype=torch.float32), persistent=False)

    def forward(self, x):
        return self.encoding(x) * self.mask

    def update_step(self, epoch, global_step, on_load_weights=False):
        self.current_level = min(self.start_level + max(int(global_step) - self.start_step, 0) // self.update_steps, self.n_level)
        self.mask[: self.current_level * self.n_features_per_level] = 1.0


class ProgressiveBandFrequency(nn.Module):
    """The reference's ProgressiveBandFrequency in plain torch ops: sin and cos of 2^k x for k < n_frequencies, each band times a mask
    that update_step opens over n_masking_step steps (all ones without masking)."""

    def __init__(self, in_channels, config):
        super().__init__()
        self.N_freqs = int(config["n_frequencies"])
        self.in_channels = self.n_input_dims = int(in_channels)
        self.funcs = [torch.sin, torch.cos]
        self.freq_bands = 2 ** torch.linspace(0, self.N_freqs - 1, self.N_freqs)
        self.n_output_dims = self.in_channels * (len(self.funcs) * self.N_freqs)
        self.n_masking_step = config.get("n_masking_step", 0)
        self.update_step(None, None)

    def forward(self, x):
        out = []
        for freq, mask in zip(self.freq_bands.tolist(), self.mask.tolist()):
            for func in self.funcs:
                out.append(func(freq * x) * mask)
        return torch.cat(out, -1)

    def update_step(self, epoch, global_step, on_load_weights=False):
        if self.n_masking_step <= 0 or global_step is None:
            self.mask = torch.ones(self.N_freqs, dtype=torch.float32)
        else:
            self.mask = (1.0 - torch.cos(math.pi * (global_step / self.n_masking_step * self.N_freqs -
                                                    torch.arange(0, self.N_freqs)).clamp(0, 1))) / 2.0


class CompositeEncoding(nn.Module):
    """The reference's CompositeEncoding: the wrapped encoding, behind x * xyz_scale + xyz_offset when include_xyz."""

    def __init__(self, encoding, include_xyz=False, xyz_scale=2.0, xyz_offset=-1.0):
        super().__init__()
        self.encoding = encoding
        self.include_xyz, self.xyz_scale, self.xyz_offset = bool(include_xyz), xyz_scale, xyz_offset
        self.n_input_dims = encoding.n_input_dims
        self.n_output_dims = int(self.include_xyz) * encoding.n_input_dims + encoding.n_output_dims

    def forward(self, x, *args):
        if not self.include_xyz:
            return self.encoding(x, *args)
        return torch.cat([x * self.xyz_scale + self.xyz_offset, self.encoding(x, *args)], dim=-1)

    def update_step(self, epoch, global_step, on_load_weights=False):
        if hasattr(self.encoding, "update_step"):
            self.encoding.update_step(epoch, global_step, on_load_weights)


_ACTIVATIONS = {"none": lambda x: x, "sigmoid": torch.sigmoid, "tanh": torch.tanh, "relu": torch.relu, "exp": torch.exp,
                "softplus": nn.functional.softplus}


def get_activation(name):
    """The output activations of the reference's get_activation that the project uses: None / "none", sigmoid, tanh, relu, exp, softplus."""
    key = "none" if name is None else str(name).lower()
    if key not in _ACTIVATIONS:
        raise ValueError("unknown activation %r; supported: %s" % (name, sorted(_ACTIVATIONS)))
    return _ACTIVATIONS[key]


class VanillaMLP(nn.Module):
    """The reference's VanillaMLP: n_hidden_layers bias-free nn.Linear of n_neurons with ReLU, a bias-free output layer and
    output_activation, in float32 whatever autocast says."""

    def __init__(self, dim_in, dim_out, config):
        super().__init__()
        self.n_neurons, self.n_hidden_layers = int(config["n_neurons"]), int(config["n_hidden_layers"])
        if self.n_neurons < 1 or self.n_hidden_layers < 1:
            raise ValueError("VanillaMLP: n_neurons and n_hidden_layers must be at least 1")
        if str(config.get("activation", "ReLU")).lower() != "relu":
            raise ValueError("VanillaMLP: the hidden activation is ReLU, not %r" % (config.get("activation"),))
        layers = [nn.Linear(int(dim_in), self.n_neurons, bias=False), nn.ReLU(inplace=True)]
        for _ in range(self.n_hidden_layers - 1):
            layers += [nn.Linear(self.n_neurons, self.n_neurons, bias=False), nn.ReLU(inplace=True)]
        layers.append(nn.Linear(self.n_neurons, int(dim_out), bias=False))
        self.layers = nn.Sequential(*layers)
        self.output_activation = get_activation(config.get("output_activation", None))

    def forward(self, x):
        with torch.autocast(device_type=x.device.type, enabled=False):
            return self.output_activation(self.layers(x))


def _otype(config, supported, what):
    if not isinstance(config, dict):
        raise ValueError("%s: the configuration must be a dict" % what)
    otype = config.get("otype")
    if otype == "Grid" and config.get("type", "Hash") == "Hash" and "HashGrid" in supported:
        otype = "HashGrid"
    if otype not in supported:
        raise ValueError("%s: unknown otype %r; supported: %s" % (what, config.get("otype"), ", ".join(supported)))
    return otype


def get_encoding(n_input_dims, config):
    """The reference's get_encoding for a dict: HashGrid, ProgressiveBandHashGrid or ProgressiveBandFrequency, wrapped in a
    CompositeEncoding (include_xyz from the configuration).  The input is supposed to lie in [0, 1]."""
    otype = _otype(config, ENCODING_OTYPES, "get_encoding")
    if otype == "ProgressiveBandFrequency":
        encoding = ProgressiveBandFrequency(n_input_dims, config)
    elif otype == "ProgressiveBandHashGrid":
        encoding = ProgressiveBandHashGrid(n_input_dims, config)
    else:
        encoding = HashGridEncoding(n_input_dims, config)
    return CompositeEncoding(encoding, include_xyz=config.get("include_xyz", False), xyz_scale=2.0, xyz_offset=-1.0)


def get_mlp(n_input_dims, n_output_dims, config):
    """The reference's get_mlp for a dict: VanillaMLP."""
    _otype(config, MLP_OTYPES, "get_mlp")
    return VanillaMLP(n_input_dims, n_output_dims, config)
