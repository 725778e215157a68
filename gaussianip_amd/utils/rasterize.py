"""A triangle rasterizer for the exported mesh (csrc/mesh_raster.hip, gip_mesh_*): the reference's nvdiffrast wrapper
(threestudio/utils/rasterize.py, NVDiffRasterizerContext) on gfx950, and render_mesh, which draws what
GaussianModel.extract_textured_mesh returns from a Camera.

Conventions (the kernel file's header states the whole definition): positions are clip space, pos [B, V, 4]; pixel (px, py) has its
centre at NDC ((2 px + 1) / W - 1, (2 py + 1) / H - 1) and the row index grows with NDC y, as in the Gaussian rasterizer, so
`verts_h @ camera.full_proj_transform` lands pixel for pixel on the Gaussian render.  rast [B, H, W, 4] = (u, v, z/w, triangle index
+ 1), zeros where nothing is drawn.  There is no polygon clipping: a triangle with a vertex at w <= 0 (behind the camera) or beyond the
guard band is dropped whole, which an orbit camera around an avatar never meets.  The forward is bit-reproducible.  Gradients reach
attributes and textures through float atomic adds, so the backward is not bit-reproducible.

Gradients to vertex positions and the antialias pass (csrc/mesh_grad.hip) are opt-in: DiffMeshRasterizerContext, and the keywords
position_gradients / antialias of render_mesh.  There rast carries a gradient to pos (the snapping is straight-through), interpolate
and the fused shade are differentiable in rast, and antialias blends across silhouette edges, which is the one route by which a loss
on coverage reaches the geometry.  The default MeshRasterizerContext and the default keywords behave as they always did and raise
NotImplementedError when asked for either.

Pixel differentials and mipmaps (csrc/mesh_mip.hip) are opt-in in the same way: MipMeshRasterizerContext returns rast_db from
rasterize, takes rast_db / diff_attrs in interpolate and uv_da / mip_level_bias / mip / max_mip_level and the mipmap filter modes in
texture, with their gradients.  The two other contexts raise NotImplementedError naming the argument when asked for any of them, and
render_mesh stays bilinear: the baked atlas gives every face its own cell, and a mip level above 0 would mix unrelated faces.

The regularisers that a loss on render_mesh(position_gradients=True) needs beside it (vertex normals, Laplacian, normal consistency) are
in utils/mesh_geometry.py (csrc/mesh_geom.hip).

render_field_mesh draws a geometry that carries a feature network (utils/isosurface.py TetrahedraSDFGrid with n_feature_dims=3, whose
colour is a hash-grid encoding and an MLP: utils/encoding.py) the way the reference's nvdiff-rasterizer does.
"""
import ctypes

import torch

from .. import _lib
from .._lib import call_model, ptr

__all__ = ["MeshRasterizerContext", "DiffMeshRasterizerContext", "MipMeshRasterizerContext", "MipStack", "edge_topology", "render_mesh",
           "render_field_mesh"]


_MAX_SIDE = 16384             # of an image or a texture: the library's MR_MAX_SIZE
_INT32_MAX = 2 ** 31 - 1      # the most pixels, or values of one tensor, the library indexes


def _is_gpu_float(t):
    return isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32


def _gpu_float(t, what, dims, last=None):
    if not (_is_gpu_float(t) and t.dim() in dims and (last is None or t.shape[-1] == last)):
        raise ValueError("%s must be a float32 GPU tensor with %s dimensions%s" %
                         (what, " or ".join(str(d) for d in dims), "" if last is None else " and a last dimension of %d" % last))
    return t.detach().contiguous()


def _resolution(resolution):
    if isinstance(resolution, (tuple, list)):
        if len(resolution) != 2:
            raise ValueError("resolution must be an int or (H, W)")
        H, W = int(resolution[0]), int(resolution[1])
    else:
        H = W = int(resolution)
    if H < 1 or W < 1 or H > _MAX_SIDE or W > _MAX_SIDE:
        raise ValueError("resolution must lie in 1 .. %d" % _MAX_SIDE)
    return H, W


def _index_tensor(tri, what, limit, validate=True):
    """[F, 3] int32 GPU indices.  validate: one host read checks that all lie inside [0, limit) (ValueError otherwise).  A caller that
    knows its indices, such as the faces extract_mesh returned, passes validate=False and saves the synchronisation; the kernels
    drop a triangle whose index is out of range, so memory safety does not depend on the check."""
    if not (isinstance(tri, torch.Tensor) and tri.is_cuda and tri.dtype == torch.int32 and tri.dim() == 2 and tri.shape[1] == 3):
        raise ValueError("%s must be an [F, 3] int32 GPU tensor" % what)
    if validate and tri.shape[0]:
        lo, hi = (int(x) for x in torch.stack((tri.min(), tri.max())).cpu())
        if lo < 0 or hi >= limit:
            raise ValueError("%s: indices must lie in [0, %d)" % (what, limit))
    return tri.detach().contiguous()


def _workspace_bytes(B, H, W, F):
    """gip_mesh_raster_workspace_size's formula (tests/test_mesh_render_cpu.py holds the two together): the [B, H, W] keys of 8 bytes,
    16 bytes of list count, the list of B * F int32.  gip_mesh_rasterize checks the shape limits and the size itself."""
    return B * H * W * 8 + 16 + B * F * 4


def _no_position_gradient(t, what):
    if isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("%s requires a gradient, and no gradient reaches vertex positions: pass %s.detach()" % (what, what))


def _rasterize(pos, tri, resolution, cull_backfaces=False, validate=True, differentiable=False):
    """rast of the forward kernels.  differentiable: a pos that requires a gradient goes through _RasterizeGrad (the same launch)."""
    given = pos
    if not differentiable:
        _no_position_gradient(pos, "pos")
    pos = _gpu_float(pos, "pos", (3,), 4)
    if pos.shape[0] < 1:
        raise ValueError("pos must be [B, V, 4] with B >= 1")
    B, V = int(pos.shape[0]), int(pos.shape[1])
    tri = _index_tensor(tri, "tri", V, validate)
    if tri.device != pos.device:
        raise ValueError("pos and tri must live on the same device")
    H, W = _resolution(resolution)
    F = int(tri.shape[0])
    if F == 0:      # nothing to draw: no launch
        return torch.zeros((B, H, W, 4), dtype=torch.float32, device=pos.device)
    if B * H * W > _INT32_MAX or F > 2 ** 24 - 1 or B * F > _INT32_MAX:
        raise ValueError("rasterize: %d views of %d x %d with %d triangles are outside the limits of gip_mesh_rasterize" % (B, H, W, F))
    if differentiable and given.requires_grad and torch.is_grad_enabled():
        return _RasterizeGrad.apply(given, tri, H, W, bool(cull_backfaces))
    return _rasterize_launch(pos, tri, H, W, cull_backfaces)


def _rasterize_launch(pos, tri, H, W, cull_backfaces):
    B, V, F = int(pos.shape[0]), int(pos.shape[1]), int(tri.shape[0])
    need = _workspace_bytes(B, H, W, F)
    ws = torch.empty(need, dtype=torch.uint8, device=pos.device)
    rast = torch.empty((B, H, W, 4), dtype=torch.float32, device=pos.device)
    call_model(pos.device, "gip_mesh_rasterize", ptr(pos), ptr(tri), B, V, F, H, W, int(bool(cull_backfaces)), ptr(ws), need, ptr(rast))
    return rast


class _RasterizeGrad(torch.autograd.Function):
    """The same launch, so the same rast bit for bit, with gip_mesh_rasterize_backward as its backward."""

    @staticmethod
    def forward(ctx, pos, tri, H, W, cull_backfaces):
        pos = pos.detach().contiguous()
        rast = _rasterize_launch(pos, tri, H, W, cull_backfaces)
        ctx.save_for_backward(pos, rast, tri)
        return rast

    @staticmethod
    def backward(ctx, g):
        pos, rast, tri = ctx.saved_tensors
        B, H, W, _ = rast.shape
        V, F = int(pos.shape[1]), int(tri.shape[0])
        g = g.contiguous().float()
        g_pos = torch.zeros_like(pos)
        call_model(pos.device, "gip_mesh_rasterize_backward", ptr(pos), ptr(tri), B, V, F, H, W, ptr(rast), ptr(g), ptr(g_pos))
        return g_pos, None, None, None, None


def _rast_tensor(rast):
    return _gpu_float(rast, "rast", (4,), 4)


class _Interpolate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, attr, rast, idx, F):
        B, H, W, _ = rast.shape
        nb, N, C = attr.shape
        out = torch.empty((B, H, W, C), dtype=torch.float32, device=rast.device)
        call_model(rast.device, "gip_mesh_interpolate", ptr(attr), nb, N, C, ptr(idx), F, ptr(rast), B, H, W, ptr(out))
        ctx.save_for_backward(rast, idx, attr)
        ctx.shape, ctx.F = (nb, N, C), F
        return out

    @staticmethod
    def backward(ctx, g):
        rast, idx, attr = ctx.saved_tensors
        nb, N, C = ctx.shape
        B, H, W, _ = rast.shape
        g = g.contiguous().float()
        g_attr = g_rast = None
        if ctx.needs_input_grad[0]:
            g_attr = torch.empty((nb, N, C), dtype=torch.float32, device=rast.device)
            call_model(rast.device, "gip_mesh_interpolate_backward", ptr(g), nb, N, C, ptr(idx), ctx.F, ptr(rast), B, H, W, ptr(g_attr))
        if ctx.needs_input_grad[1]:      # only a rast of DiffMeshRasterizerContext carries a gradient
            g_rast = torch.empty_like(rast)
            call_model(rast.device, "gip_mesh_interpolate_backward_rast", ptr(g), ptr(attr), nb, N, C, ptr(idx), ctx.F, ptr(rast), B, H, W,
                       ptr(g_rast))
        return g_attr, g_rast, None, None


class _Texture(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tex, uv):
        nb, Th, Tw, C = tex.shape
        B, H, W, _ = uv.shape
        out = torch.empty((B, H, W, C), dtype=torch.float32, device=uv.device)
        call_model(uv.device, "gip_mesh_texture", ptr(tex), nb, Th, Tw, C, ptr(uv), B, H, W, ptr(out))
        ctx.save_for_backward(tex, uv)
        return out

    @staticmethod
    def backward(ctx, g):
        tex, uv = ctx.saved_tensors
        nb, Th, Tw, C = tex.shape
        B, H, W, _ = uv.shape
        g = g.contiguous().float()
        g_tex = torch.empty_like(tex) if ctx.needs_input_grad[0] else None
        g_uv = torch.empty_like(uv) if ctx.needs_input_grad[1] else None
        call_model(uv.device, "gip_mesh_texture_backward", ptr(tex), nb, Th, Tw, C, ptr(uv), ptr(g), B, H, W, ptr(g_tex), ptr(g_uv))
        return g_tex, g_uv


class _Shade(torch.autograd.Function):
    """shaded [B, H, W, 4] = (r, g, b, alpha): the fused interpolate -> lookup -> composite of render_mesh."""

    @staticmethod
    def forward(ctx, tex, uv, rast, bg, flip_v):
        Th, Tw, _ = tex.shape
        B, H, W, _ = rast.shape
        F = int(uv.shape[0])
        shaded = torch.empty((B, H, W, 4), dtype=torch.float32, device=rast.device)
        call_model(rast.device, "gip_mesh_shade", ptr(rast), ptr(uv), F, int(flip_v), ptr(tex), Th, Tw, ptr(bg), B, H, W, ptr(shaded))
        ctx.save_for_backward(tex, uv, rast)
        ctx.flip_v = int(flip_v)
        return shaded

    @staticmethod
    def backward(ctx, g):
        tex, uv, rast = ctx.saved_tensors
        Th, Tw, _ = tex.shape
        B, H, W, _ = rast.shape
        F = int(uv.shape[0])
        g = g.contiguous().float()
        g_tex = torch.empty_like(tex) if ctx.needs_input_grad[0] else None
        g_uv = torch.empty_like(uv) if ctx.needs_input_grad[1] else None
        g_rast = torch.empty_like(rast) if ctx.needs_input_grad[2] else None      # render_mesh(position_gradients=True) only
        if F == 0:      # nothing was drawn: no launch
            return ((None if g_tex is None else torch.zeros_like(tex)), (None if g_uv is None else torch.zeros_like(uv)),
                    (None if g_rast is None else torch.zeros_like(rast)), None, None)
        if g_tex is not None or g_uv is not None:
            call_model(rast.device, "gip_mesh_shade_backward", ptr(rast), ptr(uv), F, ctx.flip_v, ptr(tex), Th, Tw, ptr(g), B, H, W, ptr(g_tex),
                       ptr(g_uv))
        if g_rast is not None:
            call_model(rast.device, "gip_mesh_shade_backward_rast", ptr(rast), ptr(uv), F, ctx.flip_v, ptr(tex), Th, Tw, ptr(g), B, H, W, ptr(g_rast))
        return g_tex, g_uv, g_rast, None, None


def edge_topology(tri, num_vertices):
    """topo [F, 3] int32 on tri's device (GPU or CPU), the table the antialias pass reads: for edge k of face f, the edge opposite
    corner k (from tri[f, k + 1] to tri[f, k + 2], indices mod 3), the vertex of the one other face at that edge that does not lie on
    it; -1 where no other face has the edge (a boundary); -2 where more than two faces share it (never a silhouette).

    Built from torch operations of static shape, so nothing is read back to the host: the 3 F undirected edges as 64-bit keys
    min * num_vertices + max, sorted, every key compared with its two neighbours on each side in the sorted order.  A face with a
    repeated index is not drawn (its area is zero) but is counted like any other: its two coinciding edges count as two faces at that
    edge (alone they name each other's corner, with a real neighbour the edge reads -2 for all of them), and its edge from a vertex
    to itself is a key of its own."""
    if not (isinstance(tri, torch.Tensor) and tri.dtype == torch.int32 and tri.dim() == 2 and tri.shape[1] == 3):
        raise ValueError("tri must be an [F, 3] int32 tensor")
    V = int(num_vertices)
    if V < 1 or V > _INT32_MAX:
        raise ValueError("num_vertices must lie in 1 .. 2^31 - 1")
    F = int(tri.shape[0])
    if F == 0:
        return torch.zeros((0, 3), dtype=torch.int32, device=tri.device)
    t = tri.detach().long()
    a, b = t[:, [1, 2, 0]].reshape(-1), t[:, [2, 0, 1]].reshape(-1)              # edge k of face f at 3 f + k
    key = torch.minimum(a, b) * V + torch.maximum(a, b)
    skey, order = torch.sort(key)
    pad = skey.new_full((2,), -1)
    k = torch.cat((pad, skey, pad))                                                 # k[i + 2] = skey[i]
    n = skey.shape[0]
    prev1, prev2 = k[1:n + 1] == skey, k[0:n] == skey
    next1, next2 = k[3:n + 3] == skey, k[4:n + 4] == skey
    alone = ~prev1 & ~next1
    with_next = next1 & ~prev1 & ~next2                                             # a run of exactly two, this one first
    with_prev = prev1 & ~next1 & ~prev2
    opposite = t.reshape(-1)[order]                                                 # corner k of face f: the vertex not on the edge
    o = torch.cat((opposite[:1], opposite, opposite[-1:]))
    value = torch.where(with_next, o[2:n + 2], torch.where(with_prev, o[0:n], torch.full_like(opposite, -2)))
    value = torch.where(alone, torch.full_like(value, -1), value)
    out = torch.empty_like(value)
    out[order] = value
    return out.reshape(F, 3).to(torch.int32)


class _Antialias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, color, pos, rast, tri, topo):
        B, H, W, C = color.shape
        V, F = int(pos.shape[1]), int(tri.shape[0])
        color, pos = color.detach().contiguous(), pos.detach().contiguous()
        out = torch.empty_like(color)
        call_model(color.device, "gip_mesh_antialias", ptr(color), C, ptr(rast), ptr(pos), ptr(tri), ptr(topo), B, V, F, H, W, ptr(out))
        ctx.save_for_backward(color, pos, rast, tri, topo)
        return out

    @staticmethod
    def backward(ctx, g):
        color, pos, rast, tri, topo = ctx.saved_tensors
        B, H, W, C = color.shape
        V, F = int(pos.shape[1]), int(tri.shape[0])
        g = g.contiguous().float()
        g_color = torch.empty_like(color) if ctx.needs_input_grad[0] else None
        g_pos = torch.zeros_like(pos) if ctx.needs_input_grad[1] else None
        call_model(color.device, "gip_mesh_antialias_backward", ptr(color), C, ptr(rast), ptr(pos), ptr(tri), ptr(topo), B, V, F, H, W, ptr(g),
                   ptr(g_color), ptr(g_pos))
        return g_color, g_pos, None, None, None


class _TopologyCache:
    """edge_topology of the last tri: the tensor object itself is kept and its version counter compared, so neither a tensor edited in
    place nor a new one at a freed one's address is served the old table."""

    def __init__(self):
        self.tri = self.topo = None
        self.key = None

    def get(self, tri, V):
        key = (tri._version, tuple(tri.shape), V)
        if self.tri is not tri or self.key != key:
            self.topo, self.tri, self.key = edge_topology(tri, V), tri, key
        return self.topo


def _antialias(color, rast, pos, tri, topology, cache):
    for t, what in ((color, "color"), (rast, "rast"), (pos, "pos")):
        if not _is_gpu_float(t):
            raise ValueError("%s must be a float32 GPU tensor" % what)
    if pos.dim() == 2:
        pos = pos[None]
    if pos.dim() != 3 or pos.shape[-1] != 4:
        raise ValueError("pos must be [B, V, 4] (or [V, 4])")
    if rast.dim() != 4 or rast.shape[-1] != 4 or rast.shape[0] != pos.shape[0]:
        raise ValueError("rast must be [B, H, W, 4] with pos's B")
    if color.dim() != 4 or tuple(color.shape[:3]) != tuple(rast.shape[:3]) or color.shape[3] < 1:
        raise ValueError("color must be [B, H, W, C] with rast's B, H, W and at least one channel")
    if color.numel() > _INT32_MAX:
        raise ValueError("color: at most 2^31 - 1 values")
    V = int(pos.shape[1])
    if not (isinstance(tri, torch.Tensor) and tri.is_cuda and tri.dtype == torch.int32 and tri.dim() == 2 and tri.shape[1] == 3):
        raise ValueError("tri must be an [F, 3] int32 GPU tensor")
    if tri.shape[0] == 0 or V == 0:      # nothing is drawn: nothing to blend, no launch
        return color
    if topology is None:
        topology = cache.get(tri, V)
    elif not (isinstance(topology, torch.Tensor) and topology.is_cuda and topology.dtype == torch.int32 and
              tuple(topology.shape) == tuple(tri.shape)):
        raise ValueError("topology must be what edge_topology(tri, V) returned: an [F, 3] int32 GPU tensor")
    return _Antialias.apply(color, pos, rast.detach().contiguous(), tri.detach().contiguous(), topology.contiguous())


def _texture_tensor(tex, uv=None, whole_stack=False):
    """tex as [nb, Th, Tw, C], checked against uv [B, H, W, 2] where one is given.  whole_stack: the mip stack's limit, which counts the
    values of all nb textures together."""
    if not (_is_gpu_float(tex) and tex.dim() in (3, 4)):
        raise ValueError("tex must be a float32 GPU tensor, [1 or B, Th, Tw, C] or [Th, Tw, C]")
    t = tex[None] if tex.dim() == 3 else tex
    if min(t.shape) < 1 or max(t.shape[1:3]) > _MAX_SIDE or (whole_stack and t.numel() > _INT32_MAX):
        raise ValueError("tex must have at least one texel and channel, at most %d texels a side%s" %
                         (_MAX_SIDE, " and at most 2^31 - 1 values" if whole_stack else ""))
    if uv is not None:
        if not (_is_gpu_float(uv) and uv.dim() == 4 and uv.shape[-1] == 2):
            raise ValueError("uv must be a float32 GPU tensor [B, H, W, 2]")
        if t.shape[0] not in (1, uv.shape[0]) or t.device != uv.device:
            raise ValueError("tex must have a batch of 1 or B and live on uv's device")
    return t


class MeshRasterizerContext:
    """The interface of the reference's NVDiffRasterizerContext.  context_type is accepted and ignored (there is one rasterizer).
    This default context sends no gradient to positions and has no antialias pass; DiffMeshRasterizerContext has both, and
    MipMeshRasterizerContext adds pixel differentials and mipmaps."""

    _rast_input = staticmethod(_rast_tensor)      # rast is detached here: this context sends no gradient through it

    def __init__(self, context_type=None, device="cuda"):
        self.device = torch.device(device)

    def vertex_transform(self, verts, mvp_mtx):
        """[B, V, 4] clip-space positions of verts [V, 3] under mvp_mtx [B, 4, 4] (column-vector convention: p = mvp @ (x, 1))."""
        homogeneous = torch.cat((verts, verts.new_ones((verts.shape[0], 1))), 1)
        return torch.einsum("bij,vj->bvi", mvp_mtx.to(verts.dtype), homogeneous)

    def rasterize(self, pos, tri, resolution, cull_backfaces=False, validate=True):
        """(rast [B, H, W, 4], None) of pos [B, V, 4] float32 and tri [F, 3] int32, one topology for all views; resolution an int or
        (H, W).  The second value is nvdiffrast's rast_db, which is not computed: no gradient reaches `pos`.  ValueError for CPU
        tensors, a wrong dtype or shape, or indices outside [0, V) (one host read; validate=False skips it for indices known to be
        good: the kernels drop a triangle with an index out of range)."""
        return _rasterize(pos, tri, resolution, cull_backfaces, validate), None

    def rasterize_one(self, pos, tri, resolution, cull_backfaces=False, validate=True):
        """rasterize of one view: pos [V, 4] -> (rast [H, W, 4], rast_db [H, W, 4] where rasterize returns one, else None)."""
        if not (isinstance(pos, torch.Tensor) and pos.dim() == 2):
            raise ValueError("rasterize_one needs pos as [V, 4]")
        rast, rast_db = self.rasterize(pos[None, ...], tri, resolution, cull_backfaces, validate)
        return rast[0], None if rast_db is None else rast_db[0]

    def antialias(self, color, rast, pos, tri):
        raise NotImplementedError("antialias: the mesh rasterizer has no antialiasing pass")

    def interpolate(self, attr, rast, tri, rast_db=None, diff_attrs=None):
        """(out [B, H, W, C], None): attr [1 or B, N, C] (or [N, C]) at the corners tri [F, 3] names, weighted by rast's (u, v, 1 - u -
        v); zeros at empty pixels.  `tri` may be the mesh's faces or an attribute's own index tensor of the same F.  Differentiable
        in attr (float atomic adds: not bit-reproducible)."""
        if rast_db is not None:
            raise NotImplementedError("interpolate: rast_db (pixel differentials) is not supported")
        if diff_attrs is not None:
            raise NotImplementedError("interpolate: diff_attrs (attribute pixel differentials) is not supported")
        if not (_is_gpu_float(attr) and attr.dim() in (2, 3)):
            raise ValueError("attr must be a float32 GPU tensor, [N, C] or [1 or B, N, C]")
        rast = self._rast_input(rast)
        a = attr[None] if attr.dim() == 2 else attr
        if a.shape[0] not in (1, rast.shape[0]) or a.shape[2] < 1:
            raise ValueError("attr must have a batch of 1 or B and at least one channel")
        idx = _index_tensor(tri, "tri", int(a.shape[1]))
        return _Interpolate.apply(a.contiguous(), rast, idx, int(idx.shape[0])), None

    def interpolate_one(self, attr, rast, tri, rast_db=None, diff_attrs=None):
        return self.interpolate(attr[None, ...], rast, tri, rast_db, diff_attrs)

    def texture(self, tex, uv, filter_mode="linear", uv_da=None, mip=None):
        """[B, H, W, C]: the bilinear lookup of tex [1 or B, Th, Tw, C] (or [Th, Tw, C]) at uv [B, H, W, 2]; uv (0, 0) is the corner
        of tex[0, 0], texel centres lie at (i + 0.5) / T, indices are clamped at the border.  Differentiable in tex and uv."""
        if filter_mode != "linear":
            raise NotImplementedError("texture: filter_mode %r is not supported, only 'linear' (no mipmaps)" % (filter_mode,))
        if uv_da is not None or mip is not None:
            raise NotImplementedError("texture: %s (mipmaps) is not supported" % ("uv_da" if uv_da is not None else "mip"))
        return _Texture.apply(_texture_tensor(tex, uv).contiguous(), uv.contiguous())


def _rast_with_gradient(rast):
    _rast_tensor(rast)
    return rast.contiguous()


class DiffMeshRasterizerContext(MeshRasterizerContext):
    """MeshRasterizerContext with what a loss on the geometry needs (csrc/mesh_grad.hip): the class to alias to the reference's
    NVDiffRasterizerContext wherever antialias or a gradient to vertex positions is used.  The forward results are those of the
    default context bit for bit.  Pixel differentials and mipmaps (rast_db, diff_attrs, uv_da, mip) are MipMeshRasterizerContext's."""

    _rast_input = staticmethod(_rast_with_gradient)

    def __init__(self, context_type=None, device="cuda"):
        super().__init__(context_type, device)
        self._topology = _TopologyCache()

    def rasterize(self, pos, tri, resolution, cull_backfaces=False, validate=True):
        """As MeshRasterizerContext.rasterize, and differentiable in pos: dL/dpos from dL/d(u, v, depth) of rast with float atomic adds
        (gip_mesh_rasterize_backward; the snapping to the sub-pixel grid is straight-through).  rast_db stays None."""
        return _rasterize(pos, tri, resolution, cull_backfaces, validate, differentiable=True), None

    def antialias(self, color, rast, pos, tri, topology=None):
        """[B, H, W, C]: color with every pixel pair that a silhouette edge of the nearer pixel's triangle crosses blended by where
        the edge crosses (nvdiffrast's rule; csrc/mesh_grad.hip states it).  Differentiable in color and in pos [B, V, 4]; rast and tri
        are those of rasterize.  topology: what edge_topology(tri, V) returned; None builds it and keeps it on the context for this
        tri (the same tensor object, not edited in place since)."""
        return _antialias(color, rast, pos, tri, topology, self._topology)


# ---------------------------------------------------------------------------------------------------------------- differentials, mipmaps
def _rast_db_launch(pos, tri, rast):
    B, H, W, _ = rast.shape
    V, F = int(pos.shape[1]), int(tri.shape[0])
    rast_db = torch.empty_like(rast)
    call_model(rast.device, "gip_mesh_rast_db", ptr(pos), ptr(tri), B, V, F, H, W, ptr(rast), ptr(rast_db))
    return rast_db


class _InterpolateDa(torch.autograd.Function):
    """out_da of gip_mesh_interpolate_da; differentiable in attr alone (it does not depend on u, v, and rast_db carries no gradient)."""

    @staticmethod
    def forward(ctx, attr, rast, rast_db, idx, channels, K, F):
        B, H, W, _ = rast.shape
        nb, N, C = attr.shape
        out = torch.empty((B, H, W, 2 * K), dtype=torch.float32, device=rast.device)
        call_model(rast.device, "gip_mesh_interpolate_da", ptr(attr), nb, N, C, ptr(idx), F, ptr(rast), ptr(rast_db), ptr(channels), K, B, H, W,
                   ptr(out))
        ctx.save_for_backward(rast, rast_db, idx, channels)
        ctx.shape, ctx.K, ctx.F = (nb, N, C), K, F
        return out

    @staticmethod
    def backward(ctx, g):
        rast, rast_db, idx, channels = ctx.saved_tensors
        nb, N, C = ctx.shape
        B, H, W, _ = rast.shape
        g = g.contiguous().float()
        g_attr = torch.empty((nb, N, C), dtype=torch.float32, device=rast.device)
        call_model(rast.device, "gip_mesh_interpolate_da_backward", ptr(g), nb, N, C, ptr(idx), ctx.F, ptr(rast), ptr(rast_db), ptr(channels), ctx.K,
                   B, H, W, ptr(g_attr))
        return g_attr, None, None, None, None, None, None


def _mip_levels(Th, Tw, max_mip_level):
    """(max_level as the library takes it, L, the texels of levels 1 .. L) of gip_mesh_mip_levels."""
    if max_mip_level is None:
        cap = -1
    else:
        cap = int(max_mip_level)
        if cap < 0:
            raise ValueError("max_mip_level must be None or >= 0")
    L, texels = ctypes.c_int32(0), ctypes.c_int64(0)
    _lib.query_model("gip_mesh_mip_levels", Th, Tw, cap, ctypes.byref(L), ctypes.byref(texels))      # no launch: it takes no stream
    return cap, int(L.value), int(texels.value)


class MipStack:
    """The mip levels of one texture, what MipMeshRasterizerContext.texture_construct_mip returns and texture takes as mip=.  Level 0 is
    the texture itself; `buffer` [nb, texels, C] holds levels 1 .. L one after the other (csrc/mesh_mip.hip states the rule), and
    levels() returns all of them as [nb, h, w, C] views.  The stack is a constant: gradients reach the `tex` given to texture."""

    def __init__(self, shape, max_level, L, texels, buffer):
        self.shape, self.max_level, self.L, self.texels, self.buffer = tuple(shape), max_level, L, texels, buffer

    def levels(self, tex=None):
        nb, h, w, C = self.shape
        out, off = ([] if tex is None else [tex.reshape(self.shape)]), 0
        for _ in range(self.L):
            h, w = max(h // 2, 1), max(w // 2, 1)
            out.append(self.buffer[:, off:off + h * w].reshape(nb, h, w, C))
            off += h * w
        return out


def _construct_mip(t, max_mip_level):
    nb, Th, Tw, C = (int(x) for x in t.shape)
    cap, L, texels = _mip_levels(Th, Tw, max_mip_level)
    buffer = torch.empty((nb, texels, C), dtype=torch.float32, device=t.device)
    if L:
        call_model(t.device, "gip_mesh_mip_build", ptr(t), nb, Th, Tw, C, cap, ptr(buffer), texels)
    return MipStack((nb, Th, Tw, C), cap, L, texels, buffer)


class _TextureMip(torch.autograd.Function):
    """gip_mesh_texture_mip; uv_da and bias may be None.  The gradient to tex goes through the gradient stack and its fold."""

    @staticmethod
    def forward(ctx, tex, uv, uv_da, bias, stack, nearest):
        nb, Th, Tw, C = tex.shape
        B, H, W, _ = uv.shape
        out = torch.empty((B, H, W, C), dtype=torch.float32, device=uv.device)
        call_model(uv.device, "gip_mesh_texture_mip", ptr(tex), nb, Th, Tw, C, ptr(stack.buffer), stack.texels, stack.max_level, ptr(uv), ptr(uv_da),
                   ptr(bias), int(nearest), B, H, W, ptr(out))
        ctx.save_for_backward(tex, uv, uv_da, bias)
        ctx.stack, ctx.nearest = stack, int(nearest)
        return out

    @staticmethod
    def backward(ctx, g):
        tex, uv, uv_da, bias = ctx.saved_tensors
        stack = ctx.stack
        nb, Th, Tw, C = tex.shape
        B, H, W, _ = uv.shape
        g = g.contiguous().float()
        g_tex = torch.empty_like(tex) if ctx.needs_input_grad[0] else None
        g_mip = torch.empty_like(stack.buffer) if g_tex is not None and stack.L else None
        g_uv = torch.empty_like(uv) if ctx.needs_input_grad[1] else None
        g_da = torch.empty_like(uv_da) if uv_da is not None and ctx.needs_input_grad[2] else None
        g_bias = torch.empty_like(bias) if bias is not None and ctx.needs_input_grad[3] else None
        call_model(uv.device, "gip_mesh_texture_mip_backward", ptr(tex), nb, Th, Tw, C, ptr(stack.buffer), stack.texels, stack.max_level, ptr(uv),
                   ptr(uv_da), ptr(bias), ctx.nearest, ptr(g), B, H, W, ptr(g_tex), ptr(g_mip), ptr(g_uv), ptr(g_da), ptr(g_bias))
        if g_mip is not None:
            call_model(uv.device, "gip_mesh_mip_fold", ptr(g_tex), nb, Th, Tw, C, stack.max_level, ptr(g_mip), stack.texels)
        return g_tex, g_uv, g_da, g_bias, None, None


class MipMeshRasterizerContext(DiffMeshRasterizerContext):
    """DiffMeshRasterizerContext with pixel differentials and mipmaps (csrc/mesh_mip.hip): the class to alias to the reference's
    NVDiffRasterizerContext wherever rast_db, diff_attrs or a mipmapped texture lookup is used.  rasterize returns (rast, rast_db) as
    the reference's wrapper does; rast, interpolate's first value and a "linear" lookup are the parent's, bit for bit.

    rast_db carries no gradient to pos (nvdiffrast's grad_db=False; the reference's wrapper asks for grad_db=True): a loss reaches the
    positions through rast and through antialias, as in the parent, but not through the level of detail."""

    def rasterize(self, pos, tri, resolution, cull_backfaces=False, validate=True):
        """(rast [B, H, W, 4], rast_db [B, H, W, 4]): rast as DiffMeshRasterizerContext.rasterize gives it, rast_db = (du/dX, du/dY,
        dv/dX, dv/dY) of its (u, v) in pixels (Y grows with the row index), zeros at empty pixels.  rast_db.requires_grad is False."""
        rast = _rasterize(pos, tri, resolution, cull_backfaces, validate, differentiable=True)
        if int(tri.shape[0]) == 0:      # nothing is drawn: no launch
            return rast, torch.zeros_like(rast)
        return rast, _rast_db_launch(pos.detach().contiguous(), tri.detach().contiguous(), rast.detach())

    def interpolate(self, attr, rast, tri, rast_db=None, diff_attrs=None):
        """(out, out_da).  Without rast_db and diff_attrs: the parent's (out, None).  With both: out is the parent's, bit for bit, and
        out_da [B, H, W, 2 K] holds (da/dX, da/dY) per pixel for the K channels of diff_attrs ("all", or a list of channel indices, in
        the list's order); zeros at empty pixels.  out_da is differentiable in attr (float atomic adds); nothing reaches rast or rast_db
        through it.  ValueError for one of the two without the other, an index outside [0, C) or a wrong shape."""
        if rast_db is None and diff_attrs is None:
            return super().interpolate(attr, rast, tri)
        if rast_db is None or diff_attrs is None:
            raise ValueError("interpolate: rast_db and diff_attrs go together (got only %s)" % ("diff_attrs" if rast_db is None else "rast_db"))
        out, _ = super().interpolate(attr, rast, tri)
        r = _rast_tensor(rast)
        db = _gpu_float(rast_db, "rast_db", (4,), 4)
        if tuple(db.shape) != tuple(r.shape) or db.device != r.device:
            raise ValueError("rast_db must have rast's shape [B, H, W, 4] and device")
        a = (attr[None] if attr.dim() == 2 else attr).contiguous()
        C = int(a.shape[2])
        if isinstance(diff_attrs, str):
            if diff_attrs != "all":
                raise ValueError("diff_attrs must be 'all' or a list of channel indices")
            channels, K = None, C
        else:
            chosen = [int(c) for c in diff_attrs]
            if not chosen or min(chosen) < 0 or max(chosen) >= C:
                raise ValueError("diff_attrs: channel indices must lie in [0, %d) and there must be at least one" % C)
            channels, K = torch.tensor(chosen, dtype=torch.int32, device=r.device), len(chosen)
        if r.numel() // 4 * 2 * K > _INT32_MAX:
            raise ValueError("interpolate: out_da would hold more than 2^31 - 1 values")
        idx = _index_tensor(tri, "tri", int(a.shape[1]), validate=False)      # the parent's call has checked it
        return out, _InterpolateDa.apply(a, r, db, idx, channels, K, int(idx.shape[0]))

    def texture_construct_mip(self, tex, max_mip_level=None):
        """The MipStack of tex [1 or B, Th, Tw, C] (or [Th, Tw, C]) to pass as texture(..., mip=): level l + 1 averages the 2 x 2
        blocks of level l, while every side above 1 is even, down to 1 x 1 or max_mip_level.  One call into the library."""
        return _construct_mip(_texture_tensor(tex, whole_stack=True).detach().contiguous(), max_mip_level)

    def texture(self, tex, uv, filter_mode="auto", uv_da=None, mip_level_bias=None, mip=None, max_mip_level=None, boundary_mode="clamp"):
        """[B, H, W, C]: the lookup of tex [1 or B, Th, Tw, C] (or [Th, Tw, C]) at uv [B, H, W, 2].  filter_mode "auto" is
        "linear-mipmap-linear" when uv_da or mip_level_bias is given and "linear" otherwise; "linear" is the parent's lookup;
        "linear-mipmap-nearest" takes the one nearest level.  uv_da [B, H, W, 4] = (ds/dX, ds/dY, dt/dX, dt/dY) is what
        interpolate(uv, ..., rast_db, "all") returns; mip_level_bias [B, H, W] is added to the level.  mip: a MipStack of this tex
        (texture_construct_mip), else the stack is built here, capped at max_mip_level.  Differentiable in tex, uv, uv_da and
        mip_level_bias (float atomic adds to tex); with mip= given the gradient still reaches `tex`, the stack is a constant."""
        if boundary_mode != "clamp":
            raise NotImplementedError("texture: boundary_mode %r is not supported, only 'clamp'" % (boundary_mode,))
        if filter_mode == "auto":
            filter_mode = "linear-mipmap-linear" if uv_da is not None or mip_level_bias is not None else "linear"
        if filter_mode == "linear":
            if uv_da is not None or mip_level_bias is not None or mip is not None:
                raise ValueError("texture: filter_mode 'linear' takes no uv_da, mip_level_bias or mip")
            return super().texture(tex, uv)
        if filter_mode not in ("linear-mipmap-linear", "linear-mipmap-nearest"):
            raise NotImplementedError("texture: filter_mode %r is not supported" % (filter_mode,))
        if isinstance(mip, (list, tuple)):
            raise NotImplementedError("texture: mip as a list of tensors is not supported, pass what texture_construct_mip returned")
        t = _texture_tensor(tex, uv, whole_stack=True)
        for extra, what, shape in ((uv_da, "uv_da", tuple(uv.shape[:3]) + (4,)), (mip_level_bias, "mip_level_bias", tuple(uv.shape[:3]))):
            if extra is not None and not (_is_gpu_float(extra) and tuple(extra.shape) == shape and extra.device == uv.device):
                raise ValueError("%s must be a float32 GPU tensor of shape %s" % (what, list(shape)))
        t = t.contiguous()
        if mip is None:
            stack = _construct_mip(t.detach(), max_mip_level)
        elif not isinstance(mip, MipStack):
            raise ValueError("mip must be what texture_construct_mip returned")
        else:
            stack = mip
            if stack.shape != tuple(t.shape) or stack.buffer.device != t.device:
                raise ValueError("mip was built from a texture of shape %s, tex has %s" % (list(stack.shape), list(t.shape)))
            if max_mip_level is not None and _mip_levels(int(t.shape[1]), int(t.shape[2]), max_mip_level)[1] != stack.L:
                raise ValueError("max_mip_level does not match the given mip (%d levels above 0)" % stack.L)
        return _TextureMip.apply(t, uv.contiguous(), None if uv_da is None else uv_da.contiguous(),
                                 None if mip_level_bias is None else mip_level_bias.contiguous(), stack, filter_mode == "linear-mipmap-nearest")


_render_topology = _TopologyCache()


def render_mesh(camera, vertices, faces, uv, texture, bg_color=None, cull_backfaces=False, validate=True, position_gradients=False,
                antialias=False):
    """{"image": [3, H, W], "alpha": [1, H, W], "depth": [1, H, W], "rast": [H, W, 4]} of the textured mesh that
    GaussianModel.extract_textured_mesh returns (vertices [V, 3] float32 world coordinates, faces [F, 3] int32, uv [F, 3, 2], texture
    [T, T, 3], all on the GPU), seen from `camera` (its full_proj_transform and image size): the same pixel grid as the Gaussian
    render of that camera.  A list of cameras renders as one batch, and every entry gains a leading dimension B.

    uv is in the OBJ convention of extract_textured_mesh (v = 1 - (row + 0.5) / T) and is flipped in the shade kernels.  validate=False
    skips the host read that checks the faces' indices (GaussianModel.render_textured_mesh does: its faces come from the extraction).  alpha is coverage (0 / 1),
    depth is z/w of the projection (0 where nothing is drawn), bg_color [3] defaults to black.  image, alpha and depth are views of
    the kernels' interleaved outputs (`.contiguous()` copies them).  Differentiable in texture (and in uv): float atomic adds, so the
    backward is not bit-reproducible; the forward is.  A triangle with a vertex behind the camera is dropped whole (no clipping).  Two
    calls into the library: rasterize and shade.

    By default no gradient reaches the vertices and nothing is antialiased.  position_gradients=True lets one reach `vertices`:
    through the colour (the fused shade's gradient to rast, then the rasterizer's to positions) and through depth (rast[..., 2]).
    antialias=True passes (r, g, b, alpha) through one antialias call (depth and rast are not antialiased): alpha then takes values
    between 0 and 1 at silhouettes, and with position_gradients a loss on it moves the vertices.  The edge table is built once per
    `faces` tensor."""
    many = isinstance(camera, (list, tuple))
    cams = list(camera) if many else [camera]
    if not cams:
        raise ValueError("render_mesh needs at least one camera")
    if position_gradients:
        given = vertices
        vertices = _gpu_float(vertices, "vertices", (2,), 3)
        if given.requires_grad and torch.is_grad_enabled():
            vertices = given.contiguous()
    else:
        _no_position_gradient(vertices, "vertices")
        vertices = _gpu_float(vertices, "vertices", (2,), 3)
    dev = vertices.device
    if not (_is_gpu_float(uv) and uv.dim() == 3 and tuple(uv.shape[1:]) == (3, 2)):
        raise ValueError("uv must be an [F, 3, 2] float32 GPU tensor")
    if not (_is_gpu_float(texture) and texture.dim() == 3 and texture.shape[2] == 3 and min(texture.shape[:2]) >= 1 and
            max(texture.shape[:2]) <= _MAX_SIDE):
        raise ValueError("texture must be a [Th, Tw, 3] float32 GPU tensor of at most %d texels a side" % _MAX_SIDE)
    H, W = int(cams[0].image_height), int(cams[0].image_width)
    if any((int(c.image_height), int(c.image_width)) != (H, W) for c in cams):
        raise ValueError("render_mesh: the cameras of one batch must share an image size")
    if not (isinstance(faces, torch.Tensor) and faces.dim() == 2 and uv.shape[0] == faces.shape[0]):
        raise ValueError("uv must have one [3, 2] entry per face")
    if bg_color is None:
        bg = torch.zeros(3, dtype=torch.float32, device=dev)
    else:
        bg = torch.as_tensor(bg_color, dtype=torch.float32).to(dev).reshape(-1).contiguous()
        if bg.numel() != 3:
            raise ValueError("bg_color must have 3 values")
    mvp = torch.stack([c.full_proj_transform.to(dev).float() for c in cams])               # [B, 4, 4], row-vector convention
    verts_h = torch.cat((vertices, torch.ones_like(vertices[:, :1])), 1)
    pos = torch.matmul(verts_h[None], mvp).contiguous()                                     # [B, V, 4]
    rast = _rasterize(pos, faces, (H, W), cull_backfaces, validate, differentiable=bool(position_gradients))
    shaded = _Shade.apply(texture.contiguous(), uv.contiguous(), rast, bg, 1)
    if antialias:
        shaded = _antialias(shaded, rast, pos, faces, None, _render_topology)
    out = {"image": shaded[..., :3].permute(0, 3, 1, 2), "alpha": shaded[..., 3:].permute(0, 3, 1, 2),
           "depth": rast[..., 2:3].permute(0, 3, 1, 2), "rast": rast}
    return out if many else {k: v[0] for k, v in out.items()}


def render_field_mesh(ctx, geometry, mvp_mtx, camera_positions, height, width, bg_color=None):
    """{"opacity": [B, H, W, 1], "comp_normal": [B, H, W, 3], "comp_rgb": [B, H, W, 3], "mesh": Mesh}: the forward of the reference's
    NVDiffRasterizer (threestudio/models/renderers/nvdiff_rasterizer.py) for a geometry with a feature network
    (utils.isosurface.TetrahedraSDFGrid with n_feature_dims=3), its no-material (colour = sigmoid(features)) and a solid background.
    geometry.isosurface() is extracted, transformed by mvp_mtx [B, 4, 4] (column-vector convention) and rasterized at (height, width);
    the coverage mask and the normals (in [0, 1]) are antialiased; the surface position of every covered pixel is interpolated from
    the vertices, geometry(positions) is evaluated there, and the colour, laid over bg_color [3] (black by default), is antialiased.
    ctx is a DiffMeshRasterizerContext: gradients reach the feature network through the colour, and the signed distance and the
    deformation through the positions the features are looked up at and through the antialiased silhouette.  camera_positions [B, 3]
    is the reference's argument; without a view-dependent material nothing reads it.  One host synchronisation (the covered pixels
    are gathered with a mask), as in the reference."""
    if not isinstance(ctx, DiffMeshRasterizerContext):
        raise ValueError("render_field_mesh needs a DiffMeshRasterizerContext (antialias and gradients to positions)")
    if not (_is_gpu_float(mvp_mtx) and mvp_mtx.dim() == 3 and tuple(mvp_mtx.shape[1:]) == (4, 4)):
        raise ValueError("mvp_mtx must be a [B, 4, 4] float32 GPU tensor")
    B = int(mvp_mtx.shape[0])
    if camera_positions is not None and tuple(camera_positions.shape) != (B, 3):
        raise ValueError("camera_positions must be [B, 3]")
    H, W = _resolution((height, width))
    dev = mvp_mtx.device
    if bg_color is None:
        bg = torch.zeros(3, dtype=torch.float32, device=dev)
    else:
        bg = torch.as_tensor(bg_color, dtype=torch.float32).to(dev).reshape(-1)
        if bg.numel() != 3:
            raise ValueError("bg_color must have 3 values")
    mesh = geometry.isosurface()
    if mesh.t_pos_idx.shape[0] == 0:
        raise ValueError("render_field_mesh: the geometry's surface is empty")
    v_pos_clip = ctx.vertex_transform(mesh.v_pos, mvp_mtx).contiguous()
    rast, _ = ctx.rasterize(v_pos_clip, mesh.t_pos_idx, (H, W))
    mask = rast[..., 3:] > 0
    mask_f = mask.float()
    out = {"opacity": ctx.antialias(mask_f, rast, v_pos_clip, mesh.t_pos_idx), "mesh": mesh}
    gb_normal, _ = ctx.interpolate_one(mesh.v_nrm, rast, mesh.t_pos_idx)
    gb_normal = torch.nn.functional.normalize(gb_normal, dim=-1)
    gb_normal_aa = torch.lerp(torch.zeros_like(gb_normal), (gb_normal + 1.0) / 2.0, mask_f)
    out["comp_normal"] = ctx.antialias(gb_normal_aa.contiguous(), rast, v_pos_clip, mesh.t_pos_idx)
    selector = mask[..., 0]
    gb_pos, _ = ctx.interpolate_one(mesh.v_pos, rast, mesh.t_pos_idx)
    positions = gb_pos[selector]
    rgb_fg = torch.sigmoid(geometry(positions)["features"][..., :3]).float()
    gb_rgb_fg = torch.zeros((B, H, W, 3), dtype=rgb_fg.dtype, device=dev)
    gb_rgb_fg[selector] = rgb_fg
    gb_rgb = torch.lerp(bg.expand(B, H, W, 3), gb_rgb_fg, mask_f)
    out["comp_rgb"] = ctx.antialias(gb_rgb.contiguous(), rast, v_pos_clip, mesh.t_pos_idx)
    return out
