"""The UV atlas of a baked texture (csrc/texture.hip, GaussianModel.bake_texture) and an 8-bit RGB PNG writer / reader.

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
