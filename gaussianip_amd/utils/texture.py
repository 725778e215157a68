"""The UV atlas of a baked texture (csrc/texture.hip, GaussianModel.bake_texture), the projection of rendered views onto it
(csrc/texture_project.hip: visible_depth, project_views) and an 8-bit RGB PNG writer / reader.

The atlas is a pure function of the number of faces F and the texture size T; no unwrapping library is involved.  Every face owns a
right-isosceles triangle of texels, two faces share a square cell:

  cell side c: the largest integer with 4 <= c <= T and 2 (T // c)^2 >= F;  n = T // c cells per row;  leg b = c - 3
  face f: cell q = f // 2 (row q // n, column q % n, origin (x0, y0) = (column c, row c)), half h = f & 1
  texel (x, y) (column, row; row 0 is the top image row), cell-local i = x % c, j = y % c: half (i + j >= c) of its cell; unowned
      when its cell lies beyond column or row n - 1 or its face id is >= F
  corners in texel-index coordinates (a texel's centre is an integer): half 0  v0 (x0, y0), v1 (x0 + b, y0), v2 (x0, y0 + b);
      half 1, the point reflection,  v0 (x0 + c - 1, y0 + c - 1), v1 (x0 + c - 1 - b, y0 + c - 1), v2 (x0 + c - 1, y0 + c - 1 - b)
  OBJ texture coordinates of an index-coordinate point (s, r): vt = ((s + 0.5) / T, 1 - (r + 0.5) / T); three per face, none shared
  the point of an owned texel: (li, lj) = (i, j) for half 0, (c - 1 - i, c - 1 - j) for half 1;
      p = v0 + (li / b) (v1 - v0) + (lj / b) (v2 - v0), in float32 in that operand order; past the hypotenuse (li + lj > b) this is the
      plane extrapolated, which is what a bilinear lookup near the face's edges needs (DESIGN.md "Baking a texture").
"""
import struct
import zlib

import numpy as np
import torch

from .mesh import _mesh_args


def atlas_layout(F, size):
    """(c, n, b): cell side, cells per row and leg of the atlas of F faces in a size x size texture.  ValueError when even cells of
    side 4 do not hold F faces; the message names the smallest size that does."""
    F, T = int(F), int(size)
    if F < 0 or T < 1:
        raise ValueError("atlas_layout: F must be >= 0 and size >= 1")
    need = 0                                      # the smallest n with 2 n^2 >= F
    while 2 * need * need < F:
        need += 1
    need = max(need, 1)
    c = T // need                                 # the largest c with T // c >= need
    if c < 4:
        raise ValueError("atlas_layout: %d faces do not fit a %d x %d texture; the smallest size that works is %d" % (F, T, T, 4 * need))
    return c, T // c, c - 3


def atlas_uv(F, size):
    """[F, 3, 2] float32: the OBJ texture coordinates (u, v) of every face's three corners."""
    c, n, b = atlas_layout(F, size)
    f = np.arange(int(F), dtype=np.int64)
    q, h = f // 2, f & 1
    x0, y0 = (q % n) * c, (q // n) * c
    s = np.stack((np.where(h == 0, x0, x0 + c - 1), np.where(h == 0, x0 + b, x0 + c - 1 - b), np.where(h == 0, x0, x0 + c - 1)), 1)
    r = np.stack((np.where(h == 0, y0, y0 + c - 1), np.where(h == 0, y0, y0 + c - 1), np.where(h == 0, y0 + b, y0 + c - 1 - b)), 1)
    T = float(int(size))
    return np.stack(((s + 0.5) / T, 1.0 - (r + 0.5) / T), -1).astype(np.float32).reshape(-1, 3, 2)


def _owner(F, size, xp, **kw):
    """(face id or -1 [T, T], li, lj) with the array module xp (numpy or torch)."""
    c, n, _ = atlas_layout(F, size)
    t = xp.arange(int(size), **kw)
    x, y = t[None, :], t[:, None]
    i, j = x % c, y % c
    h = (i + j >= c) * 1
    face = 2 * ((y // c) * n + x // c) + h
    owned = (x // c < n) & (y // c < n) & (face < int(F))
    face = xp.where(owned, face, xp.full_like(face, -1))
    return face, i + h * (c - 1 - 2 * i), j + h * (c - 1 - 2 * j)      # (li, lj): (i, j), or (c - 1 - i, c - 1 - j) for half 1


def texel_owner(F, size):
    """[T, T] int64 numpy: the face that owns texel [y, x], -1 for an unowned one."""
    return _owner(F, size, np, dtype=np.int64)[0]


def texel_points(vertices_normalised, faces, size):
    """(points [K, 3] float32, face [K] int64, x [K] int64, y [K] int64) of the K owned texels of the atlas of `faces` ([F, 3] integer
    tensor) over `vertices_normalised` ([V, 3] float32), in row-major order of the texture, on the vertices' device."""
    v = vertices_normalised
    F = int(faces.shape[0])
    c, _, b = atlas_layout(F, size)
    face, li, lj = _owner(F, size, torch, dtype=torch.int64, device=v.device)
    y, x = torch.nonzero(face >= 0, as_tuple=True)
    face, li, lj = face[y, x], li[y, x], lj[y, x]
    tri = faces.to(v.device).long()[face]
    v0, v1, v2 = v[tri[:, 0]], v[tri[:, 1]], v[tri[:, 2]]
    leg = torch.full((li.shape[0],), float(b), dtype=torch.float32, device=v.device)      # a tensor: a true division, as the kernel's
    a, bb = (li.float() / leg).unsqueeze(1), (lj.float() / leg).unsqueeze(1)
    return v0 + a * (v1 - v0) + bb * (v2 - v0), face, x, y


# ---------------------------------------------------------------------------------------------------------------- views
MAX_VIEWS = 64            # gip_texture_project's limit
VIEW_FLOATS = 20          # a row of the view table: full_proj_transform (16, row-major, row-vector convention), camera_center (3), pad


def pack_views(cameras, device=None):
    """[K, 20] float32: the view table of gip_texture_project, one row per camera (its full_proj_transform, its camera_center, 0)."""
    rows = []
    for cam in cameras:
        m = torch.as_tensor(cam.full_proj_transform).detach().float().reshape(-1)
        c = torch.as_tensor(cam.camera_center).detach().float().reshape(-1)
        if m.numel() != 16 or c.numel() != 3:
            raise ValueError("pack_views: a camera needs a 4 x 4 full_proj_transform and a camera_center of 3 values")
        dev = m.device if device is None else device
        rows.append(torch.cat((m.to(dev), c.to(dev), torch.zeros(1, dtype=torch.float32, device=dev))))
    if not rows:
        raise ValueError("pack_views needs at least one camera")
    return torch.stack(rows).contiguous()


def _view_size(what, cameras):
    """(K, H, W) of a list of cameras that share an image size; ValueError for K outside 1 .. 64."""
    cams = list(cameras) if isinstance(cameras, (list, tuple)) else [cameras]
    K = len(cams)
    if not 1 <= K <= MAX_VIEWS:
        raise ValueError("%s takes 1 .. %d views, not %d" % (what, MAX_VIEWS, K))
    H, W = int(cams[0].image_height), int(cams[0].image_width)
    if any((int(c.image_height), int(c.image_width)) != (H, W) for c in cams):
        raise ValueError("%s: the cameras must share an image size" % what)
    if H < 1 or W < 1 or H > 16384 or W > 16384:
        raise ValueError("%s: the image size must lie in 1 .. 16384" % what)
    return cams, K, H, W


@torch.no_grad()
def visible_depth(cameras, vertices, faces, validate=True):
    """[K, H, W] float32: the clip-space w of the mesh surface (vertices [V, 3] float32 world coordinates, faces [F, 3] int32, on the
    GPU) visible at every pixel centre of every camera, 0 where nothing is drawn: the mesh rasterizer's visibility, then the per-view
    clip w interpolated as a one-channel attribute (perspective-correct interpolation reproduces w exactly on a plane).  What
    project_views tests a texel's own w against.  Two calls into the library."""
    from .rasterize import MeshRasterizerContext
    cams, K, H, W = _view_size("visible_depth", cameras)
    vertices, faces = _mesh_args("visible_depth", vertices, faces)
    dev = vertices.device
    if faces.shape[0] == 0 or vertices.shape[0] == 0:
        return torch.zeros((K, H, W), dtype=torch.float32, device=dev)
    mvp = torch.stack([c.full_proj_transform.to(dev).float() for c in cams])               # [K, 4, 4], row-vector convention
    pos = torch.matmul(torch.cat((vertices, torch.ones_like(vertices[:, :1])), 1)[None], mvp).contiguous()
    ctx = MeshRasterizerContext(device=dev)
    rast, _ = ctx.rasterize(pos, faces, (H, W), validate=validate)
    w, _ = ctx.interpolate(pos[..., 3:4].contiguous(), rast, faces)
    return w[..., 0].contiguous()


@torch.no_grad()
def project_views(vertices, faces, texture_size, cameras, images, vis_depth, *, depth_tolerance, alphas=None, min_cos=0.2, min_alpha=0.5,
                  two_sided=True, unpremultiply=False):
    """{"color_sum": [T, T, 3], "weight_sum": [T, T], "count": [T, T] int32, "uv": [F, 3, 2], "cell": c}: the K `images` ([K, 3, H, W]
    float32, render_views' layout, with `alphas` [K, 1, H, W], ones if omitted) of `cameras` projected onto the atlas of the mesh
    (vertices [V, 3] float32 in world coordinates, faces [F, 3] int32, on the GPU).  csrc/texture_project.hip states the definition:
    a texel takes a view when its point projects inside the image, lies no further than depth_tolerance (clip w, world units for a
    camera of this project) behind vis_depth ([K, H, W], visible_depth's result) there, is seen at cos >= min_cos (|cos| when
    two_sided) and the bilinear lookup of the view's alpha is >= min_alpha; the view weighs cos^2.  unpremultiply divides the
    looked-up colour by the looked-up alpha (for renders over a black background) and needs min_alpha > 0.  The sums are raw:
    colour = color_sum / weight_sum where count > 0.  Unowned texels stay 0.  One host read (the faces' index range) and exactly one
    call of gip_texture_project.  ValueError for K outside 1 .. 64, tensors of the wrong dtype, device or shape, cameras of different
    sizes, faces that do not fit the texture or index outside [0, V)."""
    from .._lib import call_model, ptr
    cams, K, H, W = _view_size("project_views", cameras)
    min_alpha, min_cos, depth_tolerance = float(min_alpha), float(min_cos), float(depth_tolerance)
    if unpremultiply and not min_alpha > 0:
        raise ValueError("project_views: unpremultiply needs min_alpha > 0 (the colour is divided by the alpha)")
    if not depth_tolerance >= 0:
        raise ValueError("project_views: depth_tolerance must be >= 0")
    vertices, faces = _mesh_args("project_views", vertices, faces)
    dev = vertices.device

    def on_device(t, shape, what):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == dev and t.dtype == torch.float32 and tuple(t.shape) == shape):
            raise ValueError("project_views: %s must be a float32 tensor of shape %s on the vertices' device" % (what, list(shape)))
        return t.detach()
    images = on_device(images, (K, 3, H, W), "images")
    vis_depth = on_device(vis_depth, (K, H, W), "vis_depth").contiguous()
    alphas = torch.ones((K, 1, H, W), dtype=torch.float32, device=dev) if alphas is None else on_device(alphas, (K, 1, H, W), "alphas")
    V, F, T = int(vertices.shape[0]), int(faces.shape[0]), int(texture_size)
    if T < 4 or T > 16384:
        raise ValueError("project_views: texture_size must lie in 4 .. 16384")
    c, _, _ = atlas_layout(F, T)
    out = {"color_sum": torch.zeros((T, T, 3), dtype=torch.float32, device=dev), "weight_sum": torch.zeros((T, T), dtype=torch.float32, device=dev),
           "count": torch.zeros((T, T), dtype=torch.int32, device=dev), "uv": torch.from_numpy(atlas_uv(F, T)).to(dev), "cell": c}
    if F == 0:
        return out
    lo, hi = (int(x) for x in torch.stack((faces.min(), faces.max())).cpu())      # the one host read
    if lo < 0 or hi >= V:
        raise ValueError("project_views: face indices must lie in [0, %d)" % V)
    packed = torch.cat((images, alphas), 1).permute(0, 2, 3, 1).contiguous()      # [K, H, W, 4]: a bilinear tap is one 16-byte load
    table = pack_views(cams, dev)
    call_model(dev, "gip_texture_project", ptr(vertices), V, ptr(faces), F, T, c, K, ptr(table), ptr(packed), ptr(vis_depth), H, W, depth_tolerance,
               min_cos, min_alpha, int(bool(two_sided)), int(bool(unpremultiply)), ptr(out["color_sum"]), ptr(out["weight_sum"]),
               ptr(out["count"]))
    return out


# ---------------------------------------------------------------------------------------------------------------- PNG
def _chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def write_png_rgb(path, image):
    """8-bit RGB PNG of `image` ([H, W, 3], values in [0, 1]: rint(clip(x, 0, 1) * 255), as the PLY colours), row 0 on top; filter 0
    on every row, standard library only."""
    img = np.asarray(image.detach().cpu() if isinstance(image, torch.Tensor) else image, dtype=np.float64)
    if img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("write_png_rgb needs an [H, W, 3] image")
    px = np.rint(np.clip(img, 0, 1) * 255).astype(np.uint8)
    H, W = px.shape[:2]
    rows = np.zeros((H, 1 + W * 3), np.uint8)                 # a filter byte (0: none) in front of every row
    rows[:, 1:] = px.reshape(H, W * 3)
    with open(path, "wb") as out:
        out.write(b"\x89PNG\r\n\x1a\n")
        out.write(_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)))
        out.write(_chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)))
        out.write(_chunk(b"IEND", b""))


def read_png_rgb(path):
    """[H, W, 3] uint8 of a PNG that write_png_rgb wrote (8-bit RGB, not interlaced, filter 0 on every row)."""
    with open(path, "rb") as src:
        raw = src.read()
    if raw[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("%s is not a PNG file" % path)
    pos, header, data = 8, None, b""
    while pos < len(raw):
        n, tag = struct.unpack(">I", raw[pos:pos + 4])[0], raw[pos + 4:pos + 8]
        body = raw[pos + 8:pos + 8 + n]
        if struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] != (zlib.crc32(tag + body) & 0xFFFFFFFF):
            raise ValueError("%s: bad checksum in chunk %r" % (path, tag))
        if tag == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif tag == b"IDAT":
            data += body
        elif tag == b"IEND":
            break
        pos += 12 + n
    if header is None or header[2:] != (8, 2, 0, 0, 0):
        raise ValueError("%s: only 8-bit RGB without interlacing is supported" % path)
    W, H = header[:2]
    rows = np.frombuffer(zlib.decompress(data), np.uint8).reshape(H, 1 + W * 3)
    if rows[:, 0].any():
        raise ValueError("%s: only filter 0 is supported" % path)
    return rows[:, 1:].reshape(H, W, 3).copy()
