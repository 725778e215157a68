"""A trainable tetrahedral SDF grid on the GPU (csrc/mesh_tets.hip, gip_tet_*): differentiable marching tetrahedra, the reference's
MarchingTetrahedraHelper (threestudio/models/isosurface.py:69-253), the geometry of its TetrahedraSDFGrid
(threestudio/models/geometry/tetrahedra_sdf_grid.py) and the tet_sdf_diff regulariser (threestudio/utils/ops.py:302-313).  This is the
geometry that consumes the gradients of render_mesh(position_gradients=True) and of the terms of utils/mesh_geometry.py: a signed
distance and a bounded deformation per grid vertex, out of which every step extracts a mesh whose connectivity follows the distance.

The reference sorts on every call (torch.unique over the six edges of every surface tetrahedron).  A grid's connectivity never
changes, so TetGrid does the sorts once and a call is a mark launch, one scan, one host read of three totals, an emit launch, and a
gather for the backward: no float atomic anywhere, so both directions are bitwise equal from run to run (the kernel file's header
states the definitions).  There is no CPU path for the kernels: a signed distance that is not a float32 GPU tensor is an error.
TetGrid itself is plain torch and also works on CPU tensors."""
import ctypes

import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from .. import _lib
from .._lib import call_model, ptr
from .mesh_geometry import Mesh

__all__ = ["TetGrid", "marching_tetrahedra", "tet_sdf_diff", "MarchingTetrahedraHelper", "TetrahedraSDFGrid", "scale_tensor"]

_INT32_MAX = 2 ** 31 - 1
# a tetrahedron's six corner pairs, in the order of the reference's base_tet_edges
TET_EDGE_CORNERS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
# the six Kuhn tetrahedra of a cube as cube corners (bit 0 = +x, bit 1 = +y, bit 2 = +z), every row positively oriented: csrc/field.hip
KUHN_TETS = ((0, 1, 3, 7), (0, 5, 1, 7), (0, 3, 2, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 6, 4, 7))


class TetGrid:
    """A tetrahedral grid and everything that depends on its connectivity alone, built once and read by every kernel of
    csrc/mesh_tets.hip:
      vertices [Nv, 3] float32, indices [Ft, 4] int32    its own contiguous copies
      edges [Ne, 2] int64                the unique edges (a, b), a < b, in lexicographic order: the reference's all_edges, the
                                         `tet_edges` of the mesh extras; edges32 is the kernels' int32 copy
      tet_edge_ids [Ft, 6] int32         per tetrahedron the edge ids of its corner pairs, in the reference's base_tet_edges order
      vert_edge_start [Nv + 1], vert_edge_list [2 Ne] int32    per vertex its incident edges, ascending; an entry is 2 e + end, end 0
                                         where the vertex is the edge's first index and 1 where it is its second
    num_vertices, num_tets and num_edges are Python ints.  Building reads back to the host (the index range, which raises ValueError
    outside [0, Nv), and the size `unique` produces): once per grid, not per step.  2 Ne, 6 Ft and Ne + 2 Ft stay below 2^31."""

    _TABLES = ("vertices", "indices", "edges", "edges32", "tet_edge_ids", "vert_edge_start", "vert_edge_list")

    def __init__(self, vertices, indices):
        if not (isinstance(vertices, torch.Tensor) and vertices.is_floating_point() and vertices.dim() == 2 and vertices.shape[1] == 3):
            raise ValueError("vertices must be an [Nv, 3] floating-point tensor")
        if not (isinstance(indices, torch.Tensor) and indices.dtype in (torch.int32, torch.int64) and indices.dim() == 2 and
                indices.shape[1] == 4):
            raise ValueError("indices must be an [Ft, 4] int32 or int64 tensor")
        if indices.device != vertices.device:
            raise ValueError("vertices and indices must live on the same device")
        Nv, Ft = int(vertices.shape[0]), int(indices.shape[0])
        if Nv > _INT32_MAX or 6 * Ft > _INT32_MAX:
            raise ValueError("TetGrid: at most 2^31 - 1 vertices and tetrahedron edges")
        t = indices.detach().long()
        if Ft:
            lo, hi = (int(x) for x in torch.stack((t.min(), t.max())).cpu())
            if lo < 0 or hi >= Nv:
                raise ValueError("indices: every index must lie in [0, %d)" % Nv)
        self.num_vertices, self.num_tets, self.device = Nv, Ft, vertices.device
        self.vertices = vertices.detach().to(torch.float32).contiguous()
        self.indices = t.to(torch.int32).contiguous()
        pairs = t[:, [c for pair in TET_EDGE_CORNERS for c in pair]].reshape(-1, 2)          # [6 Ft, 2], tetrahedron-major
        scale = max(Nv, 1)
        key, inverse = torch.unique(pairs.min(1).values * scale + pairs.max(1).values, return_inverse=True)     # sorted: lexicographic
        self.edges = torch.stack((key // scale, key % scale), 1)
        Ne = self.num_edges = int(key.shape[0])
        if 2 * Ne > _INT32_MAX or Ne + 2 * Ft > _INT32_MAX:
            raise ValueError("TetGrid: at most 2^31 - 1 edge ends and flags")
        self.edges32 = self.edges.to(torch.int32).contiguous()
        self.tet_edge_ids = inverse.reshape(Ft, 6).to(torch.int32).contiguous()
        e = torch.arange(Ne, dtype=torch.int64, device=t.device)
        owner = torch.cat((self.edges[:, 0], self.edges[:, 1]))
        entry = torch.cat((2 * e, 2 * e + 1))
        row_key = torch.sort(owner * max(2 * Ne, 1) + entry)[0]                               # by vertex, then by edge
        self.vert_edge_list = (row_key % max(2 * Ne, 1)).to(torch.int32)
        start = torch.zeros(Nv + 1, dtype=torch.int64, device=t.device)
        if Ne:
            start[1:] = torch.cumsum(torch.bincount(owner, minlength=Nv), 0)
        self.vert_edge_start = start.to(torch.int32)

    @classmethod
    def from_npz(cls, path, device=None):
        """The grid of one of the reference's load/tets/*.npz files (`vertices` [Nv, 3], `indices` [Ft, 4])."""
        with np.load(path) as z:
            vertices, indices = torch.from_numpy(z["vertices"]).float(), torch.from_numpy(z["indices"]).long()
        if device is not None:
            vertices, indices = vertices.to(device), indices.to(device)
        return cls(vertices, indices)

    @classmethod
    def kuhn(cls, resolution, device=None):
        """The project's own grid: (R + 1)^3 vertices on [0, 1]^3, vertex (i, j, k) / R at index (i (R + 1) + j) (R + 1) + k, and every
        cube cut into the six Kuhn tetrahedra of csrc/field.hip, cube-major.  The cut is the same in every cube, so neighbouring
        tetrahedra share whole faces; every tetrahedron (a, b, c, d) has det(b - a, c - a, d - a) > 0, which is what makes the case
        table wind the faces outward for a distance that is negative inside."""
        R = int(resolution)
        if R < 1 or 6 * 6 * R ** 3 > _INT32_MAX:
            raise ValueError("TetGrid.kuhn: resolution %d is outside 1 .. 390" % R)
        n = R + 1
        line = torch.arange(n, dtype=torch.float32, device=device) / R
        vertices = torch.stack(torch.meshgrid(line, line, line, indexing="ij"), -1).reshape(-1, 3)
        cell = torch.arange(R, dtype=torch.int64, device=device)
        i, j, k = (x.reshape(-1) for x in torch.meshgrid(cell, cell, cell, indexing="ij"))
        corner = torch.tensor(KUHN_TETS, dtype=torch.int64, device=device)                  # [6, 4] cube corners
        ci, cj, ck = corner & 1, (corner >> 1) & 1, (corner >> 2) & 1
        indices = ((i[:, None, None] + ci) * n + (j[:, None, None] + cj)) * n + (k[:, None, None] + ck)
        return cls(vertices, indices.reshape(-1, 4))

    def to(self, device):
        """This grid with its tables on `device` (itself when they are there already)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device == self.device:
            return self
        other = object.__new__(TetGrid)
        other.__dict__.update(self.__dict__)
        for name in self._TABLES:
            setattr(other, name, getattr(self, name).to(device))
        other.device = device
        return other


def _check_sdf(what, sdf, grid):
    if not isinstance(grid, TetGrid):
        raise ValueError("%s: grid must be a TetGrid" % what)
    Nv = grid.num_vertices
    if not (isinstance(sdf, torch.Tensor) and sdf.is_cuda and sdf.dtype == torch.float32 and
            tuple(sdf.shape) in ((Nv,), (Nv, 1))):
        raise ValueError("%s: sdf must be an [Nv] or [Nv, 1] float32 GPU tensor, Nv = %d of the grid" % (what, Nv))
    if grid.device != sdf.device:
        raise ValueError("%s: sdf and the grid must live on the same device" % what)


class _MarchingTetrahedra(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sdf, positions, grid):
        dev = sdf.device
        s = sdf.detach().reshape(-1).contiguous()
        pos = positions.detach().contiguous()
        Nv, Ne, Ft = grid.num_vertices, grid.num_edges, grid.num_tets
        with torch.cuda.device(dev):
            flags = torch.empty(Ne + 2 * Ft, dtype=torch.int32, device=dev)
            V = F1 = F2 = 0
            if Ne:
                call_model(dev, "gip_tet_mark", ptr(s), ptr(grid.edges32), ptr(grid.indices), Nv, Ne, Ft, ptr(flags))
                scan = torch.cumsum(flags, 0, dtype=torch.int32)
                ends = torch.stack((scan[Ne - 1], scan[Ne + Ft - 1], scan[Ne + 2 * Ft - 1]))
                a, b, c = (int(n) for n in ends.cpu())                           # the host read that sizes the outputs
                V, F1, F2 = a, b - a, c - b
            v_pos = torch.empty((V, 3), dtype=torch.float32, device=dev)
            faces = torch.empty((F1 + 2 * F2, 3), dtype=torch.int32, device=dev)
            edge_vid = None
            if V:
                edge_vid = torch.empty(Ne, dtype=torch.int32, device=dev)
                call_model(dev, "gip_tet_emit", ptr(pos), ptr(s), ptr(grid.edges32), ptr(grid.indices), ptr(grid.tet_edge_ids), ptr(flags),
                           ptr(scan), Nv, Ne, Ft, V, F1, F2, ptr(v_pos), ptr(faces), ptr(edge_vid))
                ctx.save_for_backward(s, pos, edge_vid)
        ctx.grid, ctx.count, ctx.sdf_shape = grid, V, tuple(sdf.shape)
        ctx.mark_non_differentiable(faces)
        return v_pos, faces

    @staticmethod
    @once_differentiable
    def backward(ctx, g_v, _g_faces):
        grid = ctx.grid
        need_sdf, need_pos = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        Nv, dev = grid.num_vertices, grid.device
        if ctx.count == 0:                                                         # an empty mesh: zeros, and no launch
            return (torch.zeros(ctx.sdf_shape, dtype=torch.float32, device=dev) if need_sdf else None,
                    torch.zeros((Nv, 3), dtype=torch.float32, device=dev) if need_pos else None, None)
        s, pos, edge_vid = ctx.saved_tensors
        g_v = g_v.contiguous().float()
        g_sdf = torch.empty(Nv, dtype=torch.float32, device=dev)
        g_pos = torch.empty((Nv, 3), dtype=torch.float32, device=dev) if need_pos else None
        call_model(dev, "gip_tet_backward", ptr(pos), ptr(s), ptr(grid.edges32), ptr(grid.vert_edge_start), ptr(grid.vert_edge_list),
                   ptr(edge_vid), ptr(g_v), Nv, grid.num_edges, ctx.count, ptr(g_pos), ptr(g_sdf))
        return g_sdf.reshape(ctx.sdf_shape) if need_sdf else None, g_pos, None


def marching_tetrahedra(grid, sdf, positions=None):
    """(v_pos [V, 3] float32, faces [F, 3] int32): the surface sdf == 0 of the grid by marching tetrahedra, as the reference's
    MarchingTetrahedraHelper._forward extracts it, vertex for vertex and face for face.  sdf is [Nv] or [Nv, 1]; a vertex is occupied
    where sdf > 0.  positions [Nv, 3] are the grid's vertices when None, else the deformed ones.  Differentiable in sdf and in
    positions; bit-reproducible in both directions.  An sdf of one sign gives [0, 3] tensors and a backward of zeros.  Arguments are
    float32 GPU tensors on the grid's device; anything else raises ValueError.  One host read per call sizes the outputs."""
    _check_sdf("marching_tetrahedra", sdf, grid)
    if positions is None:
        positions = grid.vertices
    if not (isinstance(positions, torch.Tensor) and positions.is_cuda and positions.dtype == torch.float32 and
            tuple(positions.shape) == (grid.num_vertices, 3) and positions.device == sdf.device):
        raise ValueError("marching_tetrahedra: positions must be an [Nv, 3] float32 GPU tensor on the sdf's device")
    return _MarchingTetrahedra.apply(sdf, positions, grid)


class _TetSdfDiff(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sdf, grid):
        dev = sdf.device
        s = sdf.detach().reshape(-1).contiguous()
        Ne = grid.num_edges
        need = ctypes.c_size_t(0)
        _lib.query_model("gip_tet_workspace_size", Ne, ctypes.byref(need))
        with torch.cuda.device(dev):
            ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
            loss = torch.empty((), dtype=torch.float32, device=dev)
            count = torch.empty(1, dtype=torch.int32, device=dev)
            call_model(dev, "gip_tet_sdf_diff", ptr(s), ptr(grid.edges32), grid.num_vertices, Ne, ptr(loss), ptr(count), ptr(ws), need.value)
        ctx.save_for_backward(s, count)
        ctx.grid, ctx.sdf_shape = grid, tuple(sdf.shape)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        s, count = ctx.saved_tensors
        grid = ctx.grid
        g = g.contiguous().float()
        g_sdf = torch.empty_like(s)
        call_model(s.device, "gip_tet_sdf_diff_backward", ptr(s), ptr(grid.edges32), ptr(grid.vert_edge_start), ptr(grid.vert_edge_list),
                   ptr(count), ptr(g), grid.num_vertices, grid.num_edges, ptr(g_sdf))
        return g_sdf.reshape(ctx.sdf_shape), None


def tet_sdf_diff(vert_sdf, grid):
    """The scalar of the reference's tet_sdf_diff(vert_sdf, tet_edges) over the grid's edges: where the signs of an edge's two distances
    differ (torch.sign: an exact zero differs from both signs), the mean of bce_with_logits(s_a, s_b > 0) plus the mean of
    bce_with_logits(s_b, s_a > 0).  `grid` is a TetGrid (the reference takes its tet_edges; they are grid.edges).  A departure: with no
    such edge the reference returns NaN, the mean of nothing; this returns a zero that hangs on the graph, with a gradient of zeros.
    Differentiable in vert_sdf, bit-reproducible in both directions, and nothing is read back to the host."""
    _check_sdf("tet_sdf_diff", vert_sdf, grid)
    if grid.num_edges == 0:
        return vert_sdf.sum() * 0.0
    return _TetSdfDiff.apply(vert_sdf, grid)


def scale_tensor(dat, inp_scale, tgt_scale):
    """The reference's threestudio.utils.ops.scale_tensor: dat from the range inp_scale to the range tgt_scale, each a pair (lo, hi) of
    numbers or a [2, D] tensor; None is (0, 1)."""
    if inp_scale is None:
        inp_scale = (0, 1)
    if tgt_scale is None:
        tgt_scale = (0, 1)
    dat = (dat - inp_scale[0]) / (inp_scale[1] - inp_scale[0])
    return dat * (tgt_scale[1] - tgt_scale[0]) + tgt_scale[0]


class MarchingTetrahedraHelper(nn.Module):
    """The surface of the reference's MarchingTetrahedraHelper over marching_tetrahedra: points_range, grid_vertices, all_edges,
    normalize_grid_deformation and forward(level, deformation=None) -> utils.mesh_geometry.Mesh with the extras grid_vertices,
    tet_edges, grid_level and grid_deformation.  tets_path names one of the reference's .npz grids (at `resolution`, which then only
    sets the deformation's bound); without it the grid is TetGrid.kuhn(resolution).  The grid follows the module's device."""
    points_range = (0, 1)

    def __init__(self, resolution, tets_path=None):
        super().__init__()
        self.resolution = int(resolution)
        self.tets_path = tets_path
        self._grid = TetGrid.from_npz(tets_path) if tets_path is not None else TetGrid.kuhn(self.resolution)
        self.register_buffer("_grid_vertices", self._grid.vertices, persistent=False)

    @property
    def grid(self):
        if self._grid.device != self._grid_vertices.device:
            self._grid = self._grid.to(self._grid_vertices.device)
        return self._grid

    @property
    def grid_vertices(self):
        return self._grid_vertices

    @property
    def all_edges(self):
        return self.grid.edges

    def normalize_grid_deformation(self, grid_vertex_offsets):
        """The offsets bounded to about half a tetrahedron: tanh / resolution over the points range, left to autograd."""
        return (self.points_range[1] - self.points_range[0]) / self.resolution * torch.tanh(grid_vertex_offsets)

    def forward(self, level, deformation=None):
        grid = self.grid
        if deformation is not None:
            grid_vertices = self.grid_vertices + self.normalize_grid_deformation(deformation)
        else:
            grid_vertices = self.grid_vertices
        v_pos, t_pos_idx = marching_tetrahedra(grid, level, grid_vertices)
        return Mesh(v_pos=v_pos, t_pos_idx=t_pos_idx, grid_vertices=grid_vertices, tet_edges=grid.edges, grid_level=level,
                    grid_deformation=deformation)


class TetrahedraSDFGrid(nn.Module):
    """The geometry of the reference's TetrahedraSDFGrid: a signed distance `sdf` [Nv, 1] and a `deformation` [Nv, 3] per vertex of a
    tetrahedral grid as the trainable parameters (buffers with fix_geometry=True; deformation is None with
    isosurface_deformable_grid=False), the buffer isosurface_bbox [2, 3], initialize_shape() for "sphere" and "ellipsoid", and
    isosurface() -> Mesh in the bbox's coordinates, kept under fix_geometry.  Inside is negative.  The feature network is opt-in:
    with n_feature_dims > 0 the grid also holds `encoding` and `feature_network` (utils/encoding.py get_encoding / get_mlp; the
    configurations default to the reference's hash grid, 16 levels of 2 features in 2^19 rows, and its 64-neuron VanillaMLP), and
    forward(points) returns {"features": [..., n_feature_dims]} at points in the bbox's coordinates.  The default n_feature_dims=0 is
    the geometry alone, and forward then returns {}.  shape_init="mesh:..." is out of scope (it needs trimesh and pysdf);
    isosurface_remove_outliers=True raises NotImplementedError, since the project removes small components with utils.mesh.clean_mesh."""

    POS_ENCODING_CONFIG = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
                           "per_level_scale": 1.447269237440378}
    MLP_NETWORK_CONFIG = {"otype": "VanillaMLP", "activation": "ReLU", "output_activation": "none", "n_neurons": 64, "n_hidden_layers": 1}

    def __init__(self, isosurface_resolution=128, isosurface_deformable_grid=True, isosurface_remove_outliers=False, shape_init=None,
                 shape_init_params=None, fix_geometry=False, radius=1.0, tets_path=None, n_feature_dims=0, pos_encoding_config=None,
                 mlp_network_config=None):
        super().__init__()
        if isosurface_remove_outliers:
            raise NotImplementedError("TetrahedraSDFGrid: isosurface_remove_outliers is not offered inside isosurface(); pass the mesh "
                                      "to utils.mesh.clean_mesh(vertices, faces, min_faces=...), which drops small components on the GPU")
        self.isosurface_resolution = int(isosurface_resolution)
        self.isosurface_deformable_grid = bool(isosurface_deformable_grid)
        self.shape_init, self.shape_init_params, self.fix_geometry = shape_init, shape_init_params, bool(fix_geometry)
        r = float(radius)
        self.register_buffer("isosurface_bbox", torch.tensor([[-r, -r, -r], [r, r, r]], dtype=torch.float32))
        self.isosurface_helper = MarchingTetrahedraHelper(self.isosurface_resolution, tets_path)
        Nv = self.isosurface_helper.grid_vertices.shape[0]
        sdf, deformation = torch.zeros((Nv, 1), dtype=torch.float32), torch.zeros((Nv, 3), dtype=torch.float32)
        if not self.fix_geometry:
            self.sdf = nn.Parameter(sdf)
            self.deformation = nn.Parameter(deformation) if self.isosurface_deformable_grid else None
        else:
            self.register_buffer("sdf", sdf)
            if self.isosurface_deformable_grid:
                self.register_buffer("deformation", deformation)
            else:
                self.deformation = None
        self.n_feature_dims = int(n_feature_dims)
        if self.n_feature_dims < 0:
            raise ValueError("n_feature_dims must not be negative")
        if self.n_feature_dims > 0:
            from .encoding import get_encoding, get_mlp
            self.encoding = get_encoding(3, dict(self.POS_ENCODING_CONFIG if pos_encoding_config is None else pos_encoding_config))
            self.feature_network = get_mlp(self.encoding.n_output_dims, self.n_feature_dims,
                                           dict(self.MLP_NETWORK_CONFIG if mlp_network_config is None else mlp_network_config))
        self.mesh = None

    def forward(self, points, output_normal=False):
        """{"features": [..., n_feature_dims]} at points [..., 3] in the bbox's coordinates: the points scaled to [0, 1] by
        isosurface_bbox (the reference's contract_to_unisphere without the unbounded mode), encoded, and through the MLP.  {} for a
        grid without a feature network."""
        if self.n_feature_dims == 0:
            return {}
        if output_normal:
            raise NotImplementedError("TetrahedraSDFGrid: a normal output is not supported, as in the reference")
        unit = scale_tensor(points, self.isosurface_bbox, (0, 1))
        enc = self.encoding(unit.reshape(-1, 3))
        return {"features": self.feature_network(enc).view(*points.shape[:-1], self.n_feature_dims)}

    def initialize_shape(self):
        """sdf = the distance of shape_init at the grid's vertices in the bbox's coordinates: "sphere" with a radius (a float),
        "ellipsoid" with three semi-axes (its pseudo distance |x / size| - 1).  None leaves the grid as it is."""
        if self.shape_init is None:
            return
        if not isinstance(self.shape_init, str):
            raise ValueError("shape_init must be a string or None")
        helper = self.isosurface_helper
        points = scale_tensor(helper.grid_vertices, helper.points_range, self.isosurface_bbox)
        if self.shape_init == "ellipsoid":
            if not (hasattr(self.shape_init_params, "__len__") and len(self.shape_init_params) == 3):
                raise ValueError("shape_init 'ellipsoid' needs three semi-axes in shape_init_params")
            size = torch.as_tensor(self.shape_init_params, dtype=torch.float32).to(points.device)
            sdf = ((points / size) ** 2).sum(dim=-1, keepdim=True).sqrt() - 1.0
        elif self.shape_init == "sphere":
            if not isinstance(self.shape_init_params, float):
                raise ValueError("shape_init 'sphere' needs a float radius in shape_init_params")
            sdf = (points ** 2).sum(dim=-1, keepdim=True).sqrt() - self.shape_init_params
        elif self.shape_init.startswith("mesh:"):
            raise NotImplementedError("shape_init 'mesh:' needs trimesh and pysdf, which this project does not depend on")
        else:
            raise ValueError("Unknown shape initialization type: %s" % self.shape_init)
        self.sdf.data = sdf.to(self.sdf.data)
        self.mesh = None

    def isosurface(self):
        """The Mesh of sdf == 0 on the (deformed) grid, its vertices scaled from the helper's points range to isosurface_bbox.  Under
        fix_geometry the first mesh is kept and returned again."""
        if self.fix_geometry and self.mesh is not None:
            return self.mesh
        helper = self.isosurface_helper
        mesh = helper(self.sdf, self.deformation)
        mesh.v_pos = scale_tensor(mesh.v_pos, helper.points_range, self.isosurface_bbox)
        self.mesh = mesh
        return mesh
