"""Geometry terms of a mesh-fitting loop on the GPU (csrc/mesh_geom.hip, gip_mesh_vertex_normals / gip_mesh_laplacian_loss /
gip_mesh_normal_consistency and their backward passes): the reference's Mesh.v_nrm, Mesh.laplacian() and Mesh.normal_consistency()
(threestudio/models/mesh.py), the regularisers that keep a surface a surface while render_mesh(position_gradients=True) moves its
vertices, and a Mesh class with the reference's surface over them.

Everything is a gather over a MeshTopology, the connectivity tables built once per face list: one lane per vertex walks its row in a
fixed order, so there is no float atomic anywhere and forward and backward are bitwise equal from run to run (the kernel file's header
states the definitions).  There is no CPU path for the terms: vertices that are not a float32 GPU tensor are an error.  MeshTopology
itself is plain torch and also works on CPU tensors."""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from .._lib import call_model, ptr

__all__ = ["MeshTopology", "vertex_normals", "laplacian_loss", "normal_consistency", "Mesh"]

_INT32_MAX = 2 ** 31 - 1


def _row_starts(owner, V):
    """[V + 1] int32 offsets of the rows of a list sorted by `owner` (int64 in [0, V))."""
    start = torch.zeros(V + 1, dtype=torch.int64, device=owner.device)
    if owner.numel():
        start[1:] = torch.cumsum(torch.bincount(owner, minlength=V), 0)
    return start.to(torch.int32)


class MeshTopology:
    """The connectivity of one face list, built once and read by every kernel of csrc/mesh_geom.hip:
      faces [F, 3] int32        its own contiguous copy of the face list (the kernels take the faces from here only, so a face list that
                                disagrees with the tables cannot be passed)
      corner_start [V + 1], corner_list [3 F] int32   the corners 3 f + k grouped by the vertex they name, ascending inside a group
      nbr_start [V + 1], nbr_list [N] int32           per vertex its distinct neighbours j != i over all face edges, ascending: the
                                reference's `adj` of _laplacian_uniform without the self pairs, which cancel in its coalesce()
      edges [E, 2] int64        the reference's Mesh.edges: the 3 F undirected pairs with the smaller index first, unique, in
                                lexicographic order, INCLUDING a pair (a, a) of a face with a repeated index (it adds 0 to the
                                consistency sum and counts in its mean); num_edges = E, num_neighbours = N are Python ints.
    faces is an [F, 3] int32 or int64 tensor on the GPU or the CPU; the tables live on its device.  Building reads back to the host (the
    index range, which raises ValueError outside [0, num_vertices), and the sizes `unique` produces): once per connectivity, not per
    step.  F == 0 gives empty tables, and nothing downstream launches."""

    def __init__(self, faces, num_vertices):
        if not (isinstance(faces, torch.Tensor) and faces.dtype in (torch.int32, torch.int64) and faces.dim() == 2 and faces.shape[1] == 3):
            raise ValueError("faces must be an [F, 3] int32 or int64 tensor")
        V, F = int(num_vertices), int(faces.shape[0])
        if V < 0 or V > _INT32_MAX or 3 * F > _INT32_MAX:
            raise ValueError("MeshTopology: at most 2^31 - 1 vertices and face corners")
        dev = faces.device
        t = faces.detach().long()
        if F:
            lo, hi = (int(x) for x in torch.stack((t.min(), t.max())).cpu())
            if lo < 0 or hi >= V:
                raise ValueError("faces: indices must lie in [0, %d)" % V)
        self.num_vertices, self.num_faces, self.device = V, F, dev
        self.faces = t.to(torch.int32).contiguous()
        flat = t.reshape(-1)                                                            # corner k of face f at 3 f + k
        order = torch.sort(flat, stable=True)[1] if F else flat
        self.corner_list = order.to(torch.int32)
        self.corner_start = _row_starts(flat[order], V)
        a, b = flat, t[:, [1, 2, 0]].reshape(-1)                                        # the 3 F face edges (0, 1), (1, 2), (2, 0)
        scale = max(V, 1)
        ekey = torch.unique(torch.minimum(a, b) * scale + torch.maximum(a, b))          # sorted keys: the lexicographic order
        self.edges = torch.stack((ekey // scale, ekey % scale), 1)
        self.num_edges = int(ekey.shape[0])
        proper = ekey[self.edges[:, 0] != self.edges[:, 1]]                             # every neighbour pair once; both directions:
        lo_v, hi_v = proper // scale, proper % scale
        nkey = torch.sort(torch.cat((lo_v * scale + hi_v, hi_v * scale + lo_v)))[0]
        self.nbr_list = (nkey % scale).to(torch.int32)
        self.nbr_start = _row_starts(nkey // scale, V)
        self.num_neighbours = int(nkey.shape[0])
        if self.num_neighbours > _INT32_MAX:
            raise ValueError("MeshTopology: at most 2^31 - 1 neighbour entries")

    def to(self, device):
        """This topology with its tables on `device` (itself when they are there already)."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if device == self.device:
            return self
        other = object.__new__(MeshTopology)
        other.__dict__.update(self.__dict__)
        for name in ("faces", "corner_start", "corner_list", "nbr_start", "nbr_list", "edges"):
            setattr(other, name, getattr(self, name).to(device))
        other.device = device
        return other


def check_topology(what, vertices, topology):
    if not (isinstance(vertices, torch.Tensor) and vertices.is_cuda and vertices.dtype == torch.float32 and vertices.dim() == 2 and
            vertices.shape[1] == 3):
        raise ValueError("%s: vertices must be a [V, 3] float32 GPU tensor" % what)
    if not isinstance(topology, MeshTopology):
        raise ValueError("%s: topology must be a MeshTopology" % what)
    if int(vertices.shape[0]) != topology.num_vertices:
        raise ValueError("%s: vertices has %d rows and the topology was built for %d" % (what, int(vertices.shape[0]), topology.num_vertices))
    if topology.faces.device != vertices.device:
        raise ValueError("%s: vertices and the topology must live on the same device" % what)


def _workspace(V, dev):
    need = ctypes.c_size_t(0)
    _lib.query_model("gip_mesh_geometry_workspace_size", V, ctypes.byref(need))
    return torch.empty(need.value, dtype=torch.uint8, device=dev), need.value


class _VertexNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, topo):
        pos = vertices.detach().contiguous()
        V, F = topo.num_vertices, topo.num_faces
        n = torch.empty((V, 3), dtype=torch.float32, device=pos.device)
        length = torch.empty(V, dtype=torch.float32, device=pos.device)
        face_normals = torch.empty((F, 3), dtype=torch.float32, device=pos.device)      # the per-face pass's output, read by the gather
        call_model(pos.device, "gip_mesh_vertex_normals", ptr(pos), ptr(topo.faces), ptr(topo.corner_start), ptr(topo.corner_list), V, F,
                   ptr(face_normals), ptr(n), ptr(length))
        ctx.save_for_backward(pos, n, length)
        ctx.topo = topo
        return n

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        pos, n, length = ctx.saved_tensors
        topo = ctx.topo
        g = g.contiguous().float()
        g_s, g_pos = torch.empty_like(pos), torch.empty_like(pos)
        call_model(pos.device, "gip_mesh_vertex_normals_backward", ptr(pos), ptr(topo.faces), ptr(topo.corner_start), ptr(topo.corner_list), ptr(n),
                   ptr(length), ptr(g), topo.num_vertices, topo.num_faces, ptr(g_s), ptr(g_pos))
        return g_pos, None


class _Laplacian(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, topo):
        pos = vertices.detach().contiguous()
        V = topo.num_vertices
        unit = torch.empty_like(pos)
        loss = torch.empty((), dtype=torch.float32, device=pos.device)
        ws, need = _workspace(V, pos.device)
        call_model(pos.device, "gip_mesh_laplacian_loss", ptr(pos), ptr(topo.nbr_start), ptr(topo.nbr_list), V, topo.num_neighbours, ptr(unit),
                   ptr(loss), ptr(ws), need)
        ctx.save_for_backward(unit)
        ctx.topo = topo
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        unit, = ctx.saved_tensors
        topo = ctx.topo
        g = g.contiguous().float()
        g_pos = torch.empty_like(unit)
        call_model(unit.device, "gip_mesh_laplacian_loss_backward", ptr(unit), ptr(topo.nbr_start), ptr(topo.nbr_list), ptr(g), topo.num_vertices,
                   topo.num_neighbours, ptr(g_pos))
        return g_pos, None


class _Consistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, normals, topo):
        n = normals.detach().contiguous()
        V = topo.num_vertices
        loss = torch.empty((), dtype=torch.float32, device=n.device)
        ws, need = _workspace(V, n.device)
        call_model(n.device, "gip_mesh_normal_consistency", ptr(n), ptr(topo.nbr_start), ptr(topo.nbr_list), V, topo.num_neighbours, topo.num_edges,
                   ptr(loss), ptr(ws), need)
        ctx.save_for_backward(n)
        ctx.topo = topo
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        n, = ctx.saved_tensors
        topo = ctx.topo
        g = g.contiguous().float()
        g_n = torch.empty_like(n)
        call_model(n.device, "gip_mesh_normal_consistency_backward", ptr(n), ptr(topo.nbr_start), ptr(topo.nbr_list), ptr(g), topo.num_vertices,
                   topo.num_neighbours, topo.num_edges, ptr(g_n))
        return g_n, None


def _zero_of(vertices):
    """A scalar 0 that still hangs on vertices' graph (its gradient is zeros)."""
    return vertices.sum() * 0.0


def vertex_normals(vertices, topology):
    """n [V, 3]: the area-weighted vertex normals of the reference's Mesh.v_nrm.  The face cross products cross(p1 - p0, p2 - p0) are
    summed over a vertex's corners and normalised; a vertex whose sum has a squared length of at most 1e-20 (an isolated one, say) gets
    (0, 0, 1) and sends no gradient.  Differentiable in vertices, bit-reproducible in both directions."""
    check_topology("vertex_normals", vertices, topology)
    if topology.num_faces == 0 or topology.num_vertices == 0:      # no face: every normal is the default; no launch
        default = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float32, device=vertices.device)
        return default.expand(topology.num_vertices, 3) + vertices * 0.0
    return _VertexNormals.apply(vertices, topology)


def laplacian_loss(vertices, topology):
    """The scalar of the reference's Mesh.laplacian(): the mean over all vertices of |deg_v p_v - sum of v's neighbours| (the uniform
    Laplacian; an isolated vertex adds 0).  Differentiable in vertices, bit-reproducible in both directions."""
    check_topology("laplacian_loss", vertices, topology)
    if topology.num_faces == 0 or topology.num_vertices == 0:
        return _zero_of(vertices)
    return _Laplacian.apply(vertices, topology)


def _consistency_of(normals, topology):
    if topology.num_edges == 0 or topology.num_vertices == 0:
        return _zero_of(normals)
    return _Consistency.apply(normals, topology)


def normal_consistency(vertices, topology):
    """The scalar of the reference's Mesh.normal_consistency(): the mean over topology.edges of 1 - cos(n_a, n_b) of vertex_normals.
    Differentiable in vertices, bit-reproducible in both directions."""
    check_topology("normal_consistency", vertices, topology)
    return _consistency_of(vertex_normals(vertices, topology), topology)


class Mesh:
    """The surface of the reference's threestudio.models.mesh.Mesh over the functions above: v_pos [V, 3] float32 on the GPU, t_pos_idx
    [F, 3] int32 or int64, requires_grad, extras / add_extra, v_nrm, edges, normal_consistency(), laplacian(), set_vertex_color / v_rgb.
    The topology is built at the first use and kept; v_nrm is kept too, as in the reference.  Tangents, xatlas unwrapping and outlier
    removal raise NotImplementedError naming what the project offers instead."""

    def __init__(self, v_pos, t_pos_idx, **kwargs):
        self.v_pos = v_pos
        self.t_pos_idx = t_pos_idx
        self._v_nrm = None
        self._v_rgb = None
        self._topology = None
        self.extras = {}
        for k, v in kwargs.items():
            self.add_extra(k, v)

    def add_extra(self, k, v):
        self.extras[k] = v

    @property
    def requires_grad(self):
        return self.v_pos.requires_grad

    @property
    def topology(self):
        if self._topology is None:
            self._topology = MeshTopology(self.t_pos_idx, int(self.v_pos.shape[0]))
        return self._topology

    @property
    def v_nrm(self):
        if self._v_nrm is None:
            self._v_nrm = vertex_normals(self.v_pos, self.topology)
        return self._v_nrm

    @property
    def edges(self):
        return self.topology.edges

    @property
    def v_rgb(self):
        return self._v_rgb

    def set_vertex_color(self, v_rgb):
        assert v_rgb.shape[0] == self.v_pos.shape[0]
        self._v_rgb = v_rgb

    def normal_consistency(self):
        check_topology("normal_consistency", self.v_pos, self.topology)
        return _consistency_of(self.v_nrm, self.topology)

    def laplacian(self):
        return laplacian_loss(self.v_pos, self.topology)

    @property
    def v_tng(self):
        raise NotImplementedError("Mesh.v_tng: tangents need a UV unwrapping, which is out of scope; the project textures a mesh through "
                                  "its fixed per-face atlas (GaussianModel.extract_textured_mesh, utils.texture)")

    @property
    def v_tex(self):
        raise NotImplementedError("Mesh.v_tex: no xatlas unwrapping; use the fixed per-face atlas of GaussianModel.extract_textured_mesh")

    @property
    def t_tex_idx(self):
        raise NotImplementedError("Mesh.t_tex_idx: no xatlas unwrapping; use the fixed per-face atlas of GaussianModel.extract_textured_mesh")

    def unwrap_uv(self, xatlas_chart_options=None, xatlas_pack_options=None):
        raise NotImplementedError("Mesh.unwrap_uv: no xatlas unwrapping; use the fixed per-face atlas of GaussianModel.extract_textured_mesh")

    def remove_outlier(self, outlier_n_faces_threshold):
        raise NotImplementedError("Mesh.remove_outlier: use utils.mesh.clean_mesh(vertices, faces, min_faces=...), which drops small "
                                  "components on the GPU")
