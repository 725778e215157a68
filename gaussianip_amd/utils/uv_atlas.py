"""Unwrapping a mesh into a chart atlas on the GPU (csrc/mesh_uv.hip, whose header states every definition): continuous UVs for the
mipmapped lookup and the exported texture, the tangents that need them, and the padding of a baked texture's seams.  In place of the
reference's xatlas unwrapping (threestudio/models/mesh.py:207-250), Mesh._compute_vertex_tangent (mesh.py:162-205) and the exporter's
cv2.inpaint (threestudio/models/exporters/mesh_exporter.py:113-121).

unwrap_charts: faces are sorted into six direction classes by their (smoothed) normal, a chart is a connected set of faces of one
class, every chart is projected along its class axis at one scale for the whole atlas and the charts' rectangles are packed on
shelves.  Segmentation, bounding boxes and the texture vertices are kernels; the adjacency table is torch (face_adjacency works on CPU
tensors too) and the packer runs on the host over the chart sizes.  There is no CPU path for the kernels.

A chart's rectangle (x0, y0, w, h), in texels: w = floor((umax - umin) s) + 2 + 2 pad, and a point of the chart sits at texel-index
coordinates x = x0 + pad + (u - umin) s (a texel's centre is an integer; row 0 is the top image row).  So 0 <= x - (x0 + pad) <
floor((umax - umin) s) + 1, and both texels of the bilinear footprint, floor(x) and floor(x) + 1, lie in [x0 + pad, x0 + w - 1 - pad]:
at least `pad` texels inside the rectangle; likewise in y.  All roundings on the way to the float32 vt are monotone and, for a texture
size that is a power of two, every integer bound is a float32 the formula reaches exactly, so the invariant holds for the stored
v_tex too (with the second texel of a footprint counting only where its weight is not 0)."""
import math

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .._lib import call_model, ptr
from .mesh import settle_labels
from .mesh_geometry import Mesh, check_topology

__all__ = ["face_adjacency", "chart_sizes", "pack_charts", "search_scale", "unwrap_charts", "ChartAtlas", "vertex_tangents",
           "dilate_texture", "UVMesh"]

_ROUNDS_BATCH = 8         # label rounds per read of the `changed` flag
_SCALE_STEP = 0.9         # the scale search tries s0 * 0.9^k
_SCALE_TRIES = 200
DEFAULT_SMOOTH_ROUNDS = 4


def face_adjacency(faces):
    """face_nbr [F, 3] int32 on faces' device (GPU or CPU): entry k is the face across edge (k, k + 1 mod 3), or -1.  It is a face
    only when exactly two face edges have that undirected edge, they belong to two different faces that traverse it in opposite
    directions, and the edge is not a repeated index (a, a)."""
    if not (isinstance(faces, torch.Tensor) and faces.dtype in (torch.int32, torch.int64) and faces.dim() == 2 and faces.shape[1] == 3):
        raise ValueError("face_adjacency: faces must be an [F, 3] int32 or int64 tensor")
    F = int(faces.shape[0])
    dev = faces.device
    nbr = torch.full((3 * F,), -1, dtype=torch.int64, device=dev)
    if F == 0:
        return nbr.reshape(0, 3).to(torch.int32)
    t = faces.detach().long()
    a, b = t.reshape(-1), t[:, [1, 2, 0]].reshape(-1)                    # edge 3 f + k runs a -> b
    scale = int(t.max()) + 1
    key = torch.minimum(a, b) * scale + torch.maximum(a, b)
    order = torch.sort(key, stable=True)[1]
    _, counts = torch.unique_consecutive(key[order], return_counts=True)
    start = torch.cumsum(counts, 0) - counts
    first = start[counts == 2]
    e0, e1 = order[first], order[first + 1]
    ok = (a[e0] != b[e0]) & (a[e0] == b[e1]) & (e0 // 3 != e1 // 3)      # same undirected edge: a0 == b1 means opposite directions
    e0, e1 = e0[ok], e1[ok]
    nbr[e0] = e1 // 3
    nbr[e1] = e0 // 3
    return nbr.reshape(F, 3).to(torch.int32)


def chart_sizes(box, scale, pad):
    """(w [C], h [C]) int64 numpy: the rectangle sizes of charts with boxes box [C, 4] float32 (umin, vmin, umax, vmax) at `scale` texels
    per unit: floor((max - min) * s) + 2 + 2 pad, the product in float32."""
    box = np.asarray(box, np.float32).reshape(-1, 4)
    s = np.float32(scale)
    w = np.floor((box[:, 2] - box[:, 0]) * s).astype(np.int64) + 2 + 2 * int(pad)
    h = np.floor((box[:, 3] - box[:, 1]) * s).astype(np.int64) + 2 + 2 * int(pad)
    return w, h


def pack_charts(w, h, size):
    """[C, 4] int64 numpy rows (x0, y0, w, h) of the shelf packing of rectangles w x h into size x size, or None when they do not fit:
    the charts sorted by h descending, then by index, placed left to right; a chart that does not fit the rest of a shelf opens the
    next one below, as high as its first chart."""
    w, h = np.asarray(w, np.int64), np.asarray(h, np.int64)
    T = int(size)
    order = sorted(range(len(w)), key=lambda c: (-int(h[c]), c))
    rect = np.zeros((len(w), 4), np.int64)
    x, y, shelf = 0, 0, 0
    for c in order:
        cw, ch = int(w[c]), int(h[c])
        if cw > T:
            return None
        if x + cw > T:
            x, y = 0, y + shelf
            shelf = 0
        if shelf == 0:
            shelf = ch
        if y + ch > T:
            return None
        rect[c] = (x, y, cw, ch)
        x += cw
    return rect


def search_scale(box, area, size, pad):
    """(scale float32, rect [C, 4]): the first of s0 * 0.9^k, k = 0, 1, ..., s0 = sqrt(0.5 size^2 / area), whose rectangles pack_charts
    fits into size x size; `area` is the sum of the projected face areas (a Python float).  ValueError when none fits (the texture is
    too small for the charts' padding)."""
    T = int(size)
    s0 = math.sqrt(0.5 * T * T / area) if area > 0 else 1.0
    for k in range(_SCALE_TRIES):
        s = np.float32(s0 * _SCALE_STEP ** k)
        if not (np.isfinite(s) and s > 0):
            break
        rect = pack_charts(*chart_sizes(box, s, pad), T)
        if rect is not None:
            return s, rect
    raise ValueError("unwrap_charts: %d charts with a padding of %d do not fit a %d x %d texture" % (len(box), int(pad), T, T))


def _decode_keys(keys):
    """float32 of the order-preserving uint32 keys: mesh_key_float of csrc/mesh_common.h, the one definition, restated for the host."""
    k = np.ascontiguousarray(keys).view(np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


class ChartAtlas:
    """What unwrap_charts returns.  On the mesh's device:
      v_tex [Vt, 2] float32      OBJ texture coordinates ((x + 0.5) / T, 1 - (y + 0.5) / T) of texel-index coordinates (x, y): the
                                 convention of utils.texture.atlas_uv, so v_tex[t_tex_idx] is the `uv` of write_obj_textured,
                                 render_mesh and gip_mesh_shade, and v_tex with t_tex_idx serves the contexts' interpolate / texture
      t_tex_idx [F, 3] int32     the texture vertex of every corner
      vmapping [Vt] int32        the position vertex of every texture vertex (xatlas' vmapping); texture vertices are the distinct
                                 (chart, vertex) pairs in that order: a seam vertex has one per chart, faces of a chart share them
      face_chart [F] int32, chart_class [C] int32 (2 axis + sign), face_nbr [F, 3] int32, faces [F, 3] int32
    and on the host chart_rect [C, 4] int64 numpy (x0, y0, w, h), chart_box [C, 4] float32 numpy (umin, vmin, umax, vmax), scale
    (float, texels per unit), texture_size, pad, num_charts."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def uv(self):
        """[F, 3, 2]: the face-varying form of v_tex."""
        return self.v_tex[self.t_tex_idx.long()]

    @torch.no_grad()
    def texel_points(self, vertices):
        """(covered [T, T] bool, points [T, T, 3] float32, face [T, T] int64, -1 where not covered): the UV layout rasterised with the
        mesh rasterizer (pos = (2 u - 1, 2 v - 1, 0, 1) of v_tex, one pixel per texel) and `vertices` [V, 3] interpolated over it; row 0
        is the top image row of the texture.  No rasteriser code of its own."""
        from .rasterize import MeshRasterizerContext
        T = self.texture_size
        dev = self.v_tex.device
        if not (isinstance(vertices, torch.Tensor) and vertices.is_cuda and vertices.dtype == torch.float32 and vertices.dim() == 2 and
                vertices.shape[1] == 3 and vertices.device == dev):
            raise ValueError("texel_points: vertices must be a [V, 3] float32 tensor on the atlas' device")
        if int(self.t_tex_idx.shape[0]) == 0:
            return (torch.zeros((T, T), dtype=torch.bool, device=dev), torch.zeros((T, T, 3), dtype=torch.float32, device=dev),
                    torch.full((T, T), -1, dtype=torch.int64, device=dev))
        pos = torch.cat((self.v_tex * 2.0 - 1.0, torch.zeros_like(self.v_tex[:, :1]), torch.ones_like(self.v_tex[:, :1])), 1)[None].contiguous()
        ctx = MeshRasterizerContext(device=dev)
        rast, _ = ctx.rasterize(pos, self.t_tex_idx, (T, T), validate=False)
        attr = vertices.detach()[self.vmapping.long()].contiguous()
        points, _ = ctx.interpolate(attr, rast, self.t_tex_idx)
        face = rast[0, :, :, 3].long() - 1
        # pixel row py holds v = (py + 0.5) / T = 1 - (y + 0.5) / T: texture row y = T - 1 - py
        return (face >= 0).flip(0), points[0].flip(0).contiguous(), face.flip(0).contiguous()


def _check_mesh(what, vertices, faces):
    from .mesh import _mesh_args
    return _mesh_args(what, vertices, faces)


@torch.no_grad()
def unwrap_charts(vertices, faces, texture_size=None, *, smooth_rounds=DEFAULT_SMOOTH_ROUNDS, min_cos=0.25, pad=2, texels_per_unit=None):
    """ChartAtlas of the mesh (vertices [V, 3] float32, faces [F, 3] int32, on the GPU) in a texture_size^2 texture.
    smooth_rounds (0 .. 64): gather rounds that smooth the face normals before the classes are taken (fewer, larger charts); min_cos
    (0 .. 0.5): the share of its area every face keeps in its chart's projection at the least; pad: texels between a chart's
    triangles and the border of its rectangle.  The scale is searched (search_scale) unless texels_per_unit gives it; with
    texels_per_unit and texture_size=None the size is the smallest power of two that holds the packing, read back as .texture_size.
    Deterministic: it depends on nothing but its arguments, and two runs are bitwise equal.  Host reads: the label rounds' flag, the
    charts' boxes and the faces' projected areas.  ValueError for bad arguments, face indices outside [0, V) or charts that do not fit."""
    vertices, faces = _check_mesh("unwrap_charts", vertices, faces)
    V, F = int(vertices.shape[0]), int(faces.shape[0])
    smooth_rounds, pad, min_cos = int(smooth_rounds), int(pad), float(min_cos)
    if not 0 <= smooth_rounds <= 64:
        raise ValueError("unwrap_charts: smooth_rounds must lie in 0 .. 64")
    if not 0.0 <= min_cos <= 0.5:
        raise ValueError("unwrap_charts: min_cos must lie in 0 .. 0.5 (a face's own class keeps 1 / sqrt(3) of its area)")
    if pad < 0 or pad > 64:
        raise ValueError("unwrap_charts: pad must lie in 0 .. 64")
    if texture_size is None and texels_per_unit is None:
        raise ValueError("unwrap_charts needs texture_size or texels_per_unit")
    if texture_size is not None and not 4 <= int(texture_size) <= 16384:
        raise ValueError("unwrap_charts: texture_size must lie in 4 .. 16384")
    if texels_per_unit is not None and not (float(texels_per_unit) > 0 and math.isfinite(float(texels_per_unit))):
        raise ValueError("unwrap_charts: texels_per_unit must be positive")
    dev = vertices.device
    i32 = dict(dtype=torch.int32, device=dev)
    if F == 0:
        T = int(texture_size) if texture_size is not None else 4
        return ChartAtlas(v_tex=torch.zeros((0, 2), dtype=torch.float32, device=dev), t_tex_idx=torch.zeros((0, 3), **i32),
                          vmapping=torch.zeros(0, **i32), face_chart=torch.zeros(0, **i32), chart_class=torch.zeros(0, **i32),
                          face_nbr=torch.zeros((0, 3), **i32), faces=faces, chart_rect=np.zeros((0, 4), np.int64),
                          chart_box=np.zeros((0, 4), np.float32), scale=float(texels_per_unit or 1.0), texture_size=T, pad=pad, num_charts=0)
    lo, hi = (int(x) for x in torch.stack((faces.min(), faces.max())).cpu())
    if lo < 0 or hi >= V:
        raise ValueError("unwrap_charts: face indices must lie in [0, %d)" % V)
    face_nbr = face_adjacency(faces).contiguous()
    normals = torch.empty((F, 3), dtype=torch.float32, device=dev)
    smooth = torch.empty((2, F, 3), dtype=torch.float32, device=dev) if smooth_rounds else None
    face_class = torch.empty(F, **i32)
    call_model(dev, "gip_uv_face_classes", ptr(vertices), ptr(faces), ptr(face_nbr), V, F, smooth_rounds, min_cos, ptr(normals),
               ptr(smooth[0] if smooth_rounds else None), ptr(smooth[1] if smooth_rounds else None), ptr(face_class))
    labels = torch.arange(F, **i32)
    changed = torch.zeros(1, **i32)

    def rounds():
        call_model(dev, "gip_uv_chart_rounds", ptr(face_nbr), ptr(face_class), F, ptr(labels), ptr(changed), _ROUNDS_BATCH)
        return changed
    settle_labels(rounds, F, _ROUNDS_BATCH, "unwrap_charts: the chart labels")
    roots, face_chart = torch.unique(labels.long(), return_inverse=True)          # sorted: a chart's id is the rank of its smallest face
    C = int(roots.shape[0])
    chart_class = face_class[roots].contiguous()
    face_chart32 = face_chart.to(torch.int32).contiguous()
    keys = torch.empty((C, 4), **i32)
    keys[:, :2] = -1                                                               # 0xffffffff
    keys[:, 2:] = 0
    call_model(dev, "gip_uv_chart_boxes", ptr(vertices), ptr(faces), ptr(face_chart32), ptr(chart_class), V, F, C, ptr(keys))
    axis = (chart_class[face_chart].long() >> 1).unsqueeze(1)
    area = math.fsum((normals.gather(1, axis).abs().reshape(-1) * 0.5).cpu().tolist())      # exactly rounded: order-independent
    box = _decode_keys(keys.cpu().numpy())
    if texels_per_unit is None:
        T = int(texture_size)
        scale, rect = search_scale(box, area, T, pad)
    else:
        scale = np.float32(texels_per_unit)
        w, h = chart_sizes(box, scale, pad)
        if texture_size is not None:
            T = int(texture_size)
            rect = pack_charts(w, h, T)
        else:
            T, rect = 4, None
            while rect is None and T <= 16384:
                rect = pack_charts(w, h, T)
                T = T if rect is not None else T * 2
        if rect is None:
            raise ValueError("unwrap_charts: %d charts at %g texels per unit do not fit a texture of %d" % (C, float(scale), min(T, 16384)))
    # texture vertices: the distinct (chart, vertex) pairs, in that order
    pair = torch.unique(face_chart.repeat_interleave(3) * V + faces.long().reshape(-1), return_inverse=True)
    vt_key, t_tex_idx = pair
    Vt = int(vt_key.shape[0])
    vmapping = (vt_key % V).to(torch.int32).contiguous()
    vt_chart = (vt_key // V).to(torch.int32).contiguous()
    origin = np.stack((box[:, 0], box[:, 1], (rect[:, 0] + pad).astype(np.float32), (rect[:, 1] + pad).astype(np.float32)), 1)
    origin = torch.from_numpy(np.ascontiguousarray(origin, np.float32)).to(dev)
    v_tex = torch.empty((Vt, 2), dtype=torch.float32, device=dev)
    call_model(dev, "gip_uv_place", ptr(vertices), ptr(vmapping), ptr(vt_chart), ptr(chart_class), ptr(origin), V, Vt, C, float(scale), T, ptr(v_tex))
    return ChartAtlas(v_tex=v_tex, t_tex_idx=t_tex_idx.reshape(F, 3).to(torch.int32).contiguous(), vmapping=vmapping,
                      face_chart=face_chart32, chart_class=chart_class, face_nbr=face_nbr, faces=faces, chart_rect=rect, chart_box=box,
                      scale=float(scale), texture_size=T, pad=pad, num_charts=C)


# ---------------------------------------------------------------------------------------------------------------- tangents
class _VertexTangents(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, v_nrm, topo, v_tex, t_tex_idx):
        pos, nrm = vertices.detach().contiguous(), v_nrm.detach().contiguous()
        V, F, Vt = topo.num_vertices, topo.num_faces, int(v_tex.shape[0])
        face_tangents = torch.empty((F, 3), dtype=torch.float32, device=pos.device)
        out = torch.empty((V, 3), dtype=torch.float32, device=pos.device)
        call_model(pos.device, "gip_uv_vertex_tangents", ptr(pos), ptr(topo.faces), ptr(topo.corner_start), ptr(topo.corner_list), ptr(t_tex_idx),
                   ptr(v_tex), ptr(nrm), V, F, Vt, ptr(face_tangents), ptr(out))
        ctx.save_for_backward(nrm, face_tangents, v_tex, t_tex_idx)
        ctx.topo = topo
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        nrm, face_tangents, v_tex, t_tex_idx = ctx.saved_tensors
        topo = ctx.topo
        V, F, Vt = topo.num_vertices, topo.num_faces, int(v_tex.shape[0])
        g = g.contiguous().float()
        g_sum, g_pos, g_nrm = torch.empty_like(nrm), torch.empty_like(nrm), torch.empty_like(nrm)
        g_edge = torch.empty((F, 6), dtype=torch.float32, device=nrm.device)
        call_model(nrm.device, "gip_uv_vertex_tangents_backward", ptr(topo.faces), ptr(topo.corner_start), ptr(topo.corner_list), ptr(t_tex_idx),
                   ptr(v_tex), ptr(nrm), ptr(face_tangents), ptr(g), V, F, Vt, ptr(g_sum), ptr(g_edge), ptr(g_pos), ptr(g_nrm))
        return g_pos, g_nrm, None, None, None


def vertex_tangents(vertices, topology, v_tex, t_tex_idx, v_nrm):
    """[V, 3]: the reference's Mesh._compute_vertex_tangent (mesh.py:162-205).  Per face the tangent (e1 b.y - e2 a.y) / den of its
    position edges e and texture edges a, b, den = a.x b.y - a.y b.x clamped away from 0 to +-1e-6; per vertex the mean over its
    corners, normalised, made perpendicular to v_nrm [V, 3] and normalised again.  Differentiable in vertices and v_nrm (v_tex
    [Vt, 2] float32 and t_tex_idx [F, 3] int32 are constants), a gather in both directions: no float atomics, bitwise equal from run to
    run.  A vertex that no face names gets (1, 0, 0) and sends no gradient (the reference yields NaN there)."""
    check_topology("vertex_tangents", vertices, topology)
    dev = vertices.device
    if not (isinstance(v_nrm, torch.Tensor) and v_nrm.is_cuda and v_nrm.dtype == torch.float32 and v_nrm.shape == vertices.shape and
            v_nrm.device == dev):
        raise ValueError("vertex_tangents: v_nrm must be a [V, 3] float32 tensor on the vertices' device")
    if not (isinstance(v_tex, torch.Tensor) and v_tex.dtype == torch.float32 and v_tex.dim() == 2 and v_tex.shape[1] == 2 and
            v_tex.device == dev):
        raise ValueError("vertex_tangents: v_tex must be a [Vt, 2] float32 tensor on the vertices' device")
    if not (isinstance(t_tex_idx, torch.Tensor) and t_tex_idx.dtype in (torch.int32, torch.int64) and
            tuple(t_tex_idx.shape) == (topology.num_faces, 3) and t_tex_idx.device == dev):
        raise ValueError("vertex_tangents: t_tex_idx must be an [F, 3] integer tensor on the vertices' device")
    if topology.num_vertices == 0:
        return vertices * 0.0
    return _VertexTangents.apply(vertices, v_nrm, topology, v_tex.detach().contiguous(), t_tex_idx.detach().to(torch.int32).contiguous())


# ---------------------------------------------------------------------------------------------------------------- dilation
@torch.no_grad()
def dilate_texture(texture, mask, rounds):
    """(texture [H, W, C], mask [H, W] bool) after `rounds` rounds of seam padding, in place of the exporter's cv2.inpaint: in a round
    every unfilled texel with at least one 8-neighbour that was filled before the round becomes the mean of those neighbours (summed in
    row-major neighbour order in float32, divided by their number) and counts as filled from then on.  Texels never reached are 0,
    and so is every unfilled texel of the input.  rounds == 0 returns the inputs themselves."""
    if not (isinstance(texture, torch.Tensor) and texture.is_cuda and texture.dtype == torch.float32 and texture.dim() == 3):
        raise ValueError("dilate_texture: texture must be an [H, W, C] float32 GPU tensor")
    if not (isinstance(mask, torch.Tensor) and mask.dtype == torch.bool and mask.shape == texture.shape[:2] and mask.device == texture.device):
        raise ValueError("dilate_texture: mask must be an [H, W] bool tensor on the texture's device")
    rounds = int(rounds)
    if rounds < 0 or rounds > 1024:
        raise ValueError("dilate_texture: rounds must lie in 0 .. 1024")
    if rounds == 0:
        return texture, mask
    H, W, C = (int(x) for x in texture.shape)
    mask_a = mask.to(torch.uint8).contiguous()
    tex_a = torch.where(mask.unsqueeze(2), texture, torch.zeros_like(texture)).contiguous()
    tex_b, mask_b = torch.empty_like(tex_a), torch.empty_like(mask_a)
    call_model(texture.device, "gip_texture_dilate", ptr(tex_a), ptr(mask_a), ptr(tex_b), ptr(mask_b), H, W, C, rounds)
    return (tex_b, mask_b.bool()) if rounds & 1 else (tex_a, mask_a.bool())


# ---------------------------------------------------------------------------------------------------------------- Mesh
class UVMesh(Mesh):
    """Mesh with the four members that need an unwrapping: unwrap_uv(), v_tex, t_tex_idx and v_tng, served from a ChartAtlas.  Like the
    reference, v_tex / t_tex_idx / v_tng unwrap on first use (at texture_size 1024, or what unwrap_uv was given)."""

    def __init__(self, v_pos, t_pos_idx, **kwargs):
        super().__init__(v_pos, t_pos_idx, **kwargs)
        self._atlas = None
        self._v_tng = None

    def unwrap_uv(self, xatlas_chart_options=None, xatlas_pack_options=None, texture_size=1024, **options):
        """Unwraps with unwrap_charts(texture_size=, **options) and keeps the atlas (also returned).  The reference's two xatlas option
        dictionaries are accepted and must be empty: ValueError otherwise, since no option of xatlas has a meaning here."""
        if xatlas_chart_options or xatlas_pack_options:
            raise ValueError("UVMesh.unwrap_uv: xatlas options are not supported (%s); pass unwrap_charts' keywords instead" %
                             sorted(dict(xatlas_chart_options or {}, **dict(xatlas_pack_options or {}))))
        self._atlas = unwrap_charts(self.v_pos, self.t_pos_idx.to(torch.int32), texture_size, **options)
        self._v_tng = None
        return self._atlas

    @property
    def atlas(self):
        if self._atlas is None:
            self.unwrap_uv()
        return self._atlas

    @property
    def v_tex(self):
        return self.atlas.v_tex

    @property
    def t_tex_idx(self):
        return self.atlas.t_tex_idx

    @property
    def v_tng(self):
        if self._v_tng is None:
            self._v_tng = vertex_tangents(self.v_pos, self.topology, self.v_tex, self.t_tex_idx, self.v_nrm)
        return self._v_tng
