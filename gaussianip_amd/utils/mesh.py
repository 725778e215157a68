"""Iso-surface of a regular grid as an indexed triangle mesh (csrc/field.hip: marching tetrahedra on the Kuhn decomposition;
include/gip_model.h gip_surface_count / gip_surface_emit), and Wavefront OBJ / binary PLY writers and readers for it, with optional
per-vertex colours and normals.

The reference hands its density grid to the third-party `mcubes` (gs_renderer.py:338-340); here the surface is extracted on the
GPU.  There is no CPU path: a tensor that is not a float32 GPU tensor is an error."""
import ctypes

import numpy as np
import torch


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def extract_surface(field, threshold):
    """(vertices [V, 3] float32 in grid-index units, faces [F, 3] int32) of the surface field == threshold.

    A grid point is inside when field >= threshold; a vertex sits on a grid edge (cube edge, face diagonal or body diagonal) whose
    ends differ, at t = (threshold - f0) / (f1 - f0); normals point toward decreasing values; the surface is closed wherever it does
    not reach the grid boundary.  Vertex and face order are fixed by the grid, so two calls return identical tensors."""
    from .. import _lib
    if not (isinstance(field, torch.Tensor) and field.is_cuda and field.dtype == torch.float32 and field.dim() == 3 and
            field.shape[0] == field.shape[1] == field.shape[2]):
        raise ValueError("extract_surface needs an [R, R, R] float32 GPU tensor")
    R = int(field.shape[0])
    if R < 2 or 7 * R ** 3 > 2 ** 31 - 1:
        raise ValueError("extract_surface: resolution %d is outside 2 .. 674" % R)
    field = field.detach().contiguous()
    dev, lib = field.device, _lib.model_lib()
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        edge_flag = torch.empty(R ** 3 * 7, dtype=torch.int32, device=dev)
        tri_count = torch.empty((R - 1) ** 3, dtype=torch.int32, device=dev)
        rc = lib.gip_surface_count(_ptr(field), R, float(threshold), _ptr(edge_flag), _ptr(tri_count), stream)
        if rc != 0:
            raise RuntimeError("gip_surface_count failed with status %d" % rc)
        edge_end = torch.cumsum(edge_flag, 0, dtype=torch.int32)
        tri_end = torch.cumsum(tri_count, 0, dtype=torch.int32)
        V, F = (int(n) for n in torch.stack((edge_end[-1], tri_end[-1])).cpu())      # the host read that sizes the outputs
        vertices = torch.empty((V, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
        if V == 0 or F == 0:
            return vertices, faces
        edge_index, tri_offset = edge_end - edge_flag, tri_end - tri_count           # exclusive scans
        rc = lib.gip_surface_emit(_ptr(field), R, float(threshold), _ptr(edge_flag), _ptr(edge_index), _ptr(tri_offset), _ptr(vertices),
                                  _ptr(faces), stream)
        if rc != 0:
            raise RuntimeError("gip_surface_emit failed with status %d" % rc)
    return vertices, faces


def _array(t, dtype):
    return np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t, dtype=dtype)


def write_obj(path, vertices, faces, colors=None, normals=None):
    """Wavefront OBJ: `v x y z` lines (9 significant digits: a float32 survives the round trip), `f a b c` lines, 1-based.  With
    `colors` ([V, 3] in [0, 1]) the vertex lines become `v x y z r g b` (the common vertex-colour extension); with `normals` ([V, 3])
    the file gains one `vn` line per vertex and the faces are written `f a//a b//b c//c`."""
    v = _array(vertices, np.float32)
    f = _array(faces, np.int64) + 1
    col = None if colors is None else _array(colors, np.float32).reshape(-1, 3)
    nrm = None if normals is None else _array(normals, np.float32).reshape(-1, 3)
    if (col is not None and col.shape[0] != v.shape[0]) or (nrm is not None and nrm.shape[0] != v.shape[0]):
        raise ValueError("write_obj: colors and normals need one row per vertex")
    with open(path, "w") as out:
        out.write("# %d vertices, %d faces\n" % (v.shape[0], f.shape[0]))
        if col is None:
            out.write("".join("v %.9g %.9g %.9g\n" % (float(a), float(b), float(c)) for a, b, c in v))
        else:
            out.write("".join("v %.9g %.9g %.9g %.9g %.9g %.9g\n" % tuple(float(x) for x in row) for row in np.concatenate((v, col), 1)))
        if nrm is None:
            out.write("".join("f %d %d %d\n" % (a, b, c) for a, b, c in f))
        else:
            out.write("".join("vn %.9g %.9g %.9g\n" % (float(a), float(b), float(c)) for a, b, c in nrm))
            out.write("".join("f %d//%d %d//%d %d//%d\n" % (a, a, b, b, c, c) for a, b, c in f))


def read_obj_full(path):
    """(vertices [V, 3] float32, faces [F, 3] int32 0-based, colors [V, 3] float32 or None, normals [V, 3] float32 or None) of an OBJ
    that write_obj wrote: colours are the fourth to sixth number of the `v` lines, normals the `vn` lines."""
    v, f, c, n = [], [], [], []
    with open(path) as src:
        for line in src:
            parts = line.split()
            if not parts:
                continue
            if parts[0] == "v":
                v.append([float(x) for x in parts[1:4]])
                if len(parts) >= 7:
                    c.append([float(x) for x in parts[4:7]])
            elif parts[0] == "vn":
                n.append([float(x) for x in parts[1:4]])
            elif parts[0] == "f":
                f.append([int(x.split("/")[0]) - 1 for x in parts[1:4]])
    if c and len(c) != len(v):
        raise ValueError("%s: some vertices carry a colour and some do not" % path)
    return (np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int32).reshape(-1, 3),
            np.asarray(c, np.float32).reshape(-1, 3) if c else None, np.asarray(n, np.float32).reshape(-1, 3) if n else None)


def read_obj(path):
    """(vertices [V, 3] float32, faces [F, 3] int32, 0-based) of an OBJ that write_obj wrote; colours and normals, if the file has
    them, are left to read_obj_full."""
    return read_obj_full(path)[:2]


def write_ply_mesh(path, vertices, faces, colors=None, normals=None):
    """Binary little-endian PLY: vertex x y z float32, then nx ny nz float32 (with `normals`), then red green blue uchar (with
    `colors`, rounded from [0, 1]); face `list uchar int vertex_indices`.  The layout MeshLab and Blender read vertex colours from."""
    v = _array(vertices, np.float32).reshape(-1, 3)
    f = _array(faces, np.int32).reshape(-1, 3)
    fields, props = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")], ["property float x", "property float y", "property float z"]
    if normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        props += ["property float nx", "property float ny", "property float nz"]
    if colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        props += ["property uchar red", "property uchar green", "property uchar blue"]
    table = np.zeros(v.shape[0], dtype=fields)
    cols = [("x", "y", "z", v)]
    if normals is not None:
        cols.append(("nx", "ny", "nz", _array(normals, np.float32).reshape(-1, 3)))
    if colors is not None:
        cols.append(("red", "green", "blue", np.rint(np.clip(_array(colors, np.float64).reshape(-1, 3), 0, 1) * 255).astype(np.uint8)))
    for a, b, c, src in cols:
        if src.shape[0] != v.shape[0]:
            raise ValueError("write_ply_mesh: colors and normals need one row per vertex")
        table[a], table[b], table[c] = src[:, 0], src[:, 1], src[:, 2]
    tris = np.zeros(f.shape[0], dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    tris["n"], tris["idx"] = 3, f
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % v.shape[0]] + props + \
             ["element face %d" % f.shape[0], "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as out:
        out.write(("\n".join(header) + "\n").encode("ascii"))
        out.write(table.tobytes())
        out.write(tris.tobytes())


_PLY_TYPES = {"float": "<f4", "float32": "<f4", "uchar": "u1", "uint8": "u1", "int": "<i4", "int32": "<i4"}


def read_ply_mesh(path):
    """(vertices [V, 3] float32, faces [F, 3] int32, colors [V, 3] float32 in [0, 1] or None, normals [V, 3] float32 or None) of a
    PLY that write_ply_mesh wrote (binary little-endian, triangles only)."""
    with open(path, "rb") as src:
        if src.readline().strip() != b"ply":
            raise ValueError("%s is not a PLY file" % path)
        fmt, element, counts, vprops, fprop = None, None, {}, [], None
        while True:
            line = src.readline()
            if not line:
                raise ValueError("%s: no end_header" % path)
            parts = line.decode("ascii").split()
            if not parts or parts[0] == "comment":
                continue
            if parts[0] == "format":
                fmt = parts[1]
            elif parts[0] == "element":
                element = parts[1]
                counts[element] = int(parts[2])
            elif parts[0] == "property" and element == "vertex":
                vprops.append((parts[2], _PLY_TYPES[parts[1]]))
            elif parts[0] == "property" and element == "face":
                fprop = parts[1:]
            elif parts[0] == "end_header":
                break
        if fmt != "binary_little_endian":
            raise ValueError("unsupported PLY format %r" % fmt)
        if counts.get("face", 0) and (fprop is None or fprop[0] != "list" or _PLY_TYPES[fprop[1]] != "u1" or _PLY_TYPES[fprop[2]] != "<i4"):
            raise ValueError("%s: faces must be `list uchar int`" % path)
        nv, nf = counts.get("vertex", 0), counts.get("face", 0)
        vdt = np.dtype(vprops)
        table = np.frombuffer(src.read(nv * vdt.itemsize), dtype=vdt, count=nv)
        fdt = np.dtype([("n", "u1"), ("idx", "<i4", (3,))])
        tris = np.frombuffer(src.read(nf * fdt.itemsize), dtype=fdt, count=nf)
    if nf and (tris["n"] != 3).any():
        raise ValueError("%s: only triangles are supported" % path)
    names = set(vdt.names)
    pick = lambda keys: np.stack([table[k] for k in keys], 1)  # noqa: E731
    vertices = pick(("x", "y", "z")).astype(np.float32).reshape(-1, 3)
    normals = pick(("nx", "ny", "nz")).astype(np.float32).reshape(-1, 3) if {"nx", "ny", "nz"} <= names else None
    colors = (pick(("red", "green", "blue")).astype(np.float32) / 255).reshape(-1, 3) if {"red", "green", "blue"} <= names else None
    return vertices, tris["idx"].astype(np.int32).reshape(-1, 3), colors, normals


def write_obj_textured(path, vertices, faces, uv, texture, normals=None):
    """Wavefront OBJ with a material and a texture, the layout of the reference's exporter (threestudio/utils/saving.py:519-545):
    `path` = dir/name.obj gets `mtllib name.mtl`, `g object`, `usemtl default`, the `v` lines, `vn` lines (with `normals`, one per
    vertex) and `vt u v` lines (uv [F, 3, 2]: three per face, none shared; numbers with 9 significant digits as write_obj), then
    `f a/t/a b/t/b c/t/c` (`f a/t b/t c/t` without normals) with t = 3 f + 1 .. 3 f + 3.  dir/name.mtl holds the reference's
    statements in its order and names dir/name_kd.png, the texture ([H, W, 3] in [0, 1], row 0 on top) as an 8-bit PNG.  The
    reference calls every texture `texture_kd.*`; here the name follows the OBJ's, because two exports into one directory would
    otherwise overwrite each other's texture."""
    import os

    from .texture import write_png_rgb
    v = _array(vertices, np.float32).reshape(-1, 3)
    f = _array(faces, np.int64).reshape(-1, 3) + 1
    vt = _array(uv, np.float32).reshape(-1, 2)
    nrm = None if normals is None else _array(normals, np.float32).reshape(-1, 3)
    if vt.shape[0] != 3 * f.shape[0]:
        raise ValueError("write_obj_textured: uv needs three rows per face")
    if nrm is not None and nrm.shape[0] != v.shape[0]:
        raise ValueError("write_obj_textured: normals need one row per vertex")
    stem = os.path.splitext(os.path.abspath(path))[0]
    name = os.path.basename(stem)
    with open(path, "w") as out:
        out.write("mtllib %s.mtl\ng object\nusemtl default\n" % name)
        out.write("".join("v %.9g %.9g %.9g\n" % (float(a), float(b), float(c)) for a, b, c in v))
        if nrm is not None:
            out.write("".join("vn %.9g %.9g %.9g\n" % (float(a), float(b), float(c)) for a, b, c in nrm))
        out.write("".join("vt %.9g %.9g\n" % (float(a), float(b)) for a, b in vt))
        if nrm is None:
            out.write("".join("f %d/%d %d/%d %d/%d\n" % (a, 3 * i + 1, b, 3 * i + 2, c, 3 * i + 3) for i, (a, b, c) in enumerate(f)))
        else:
            out.write("".join("f %d/%d/%d %d/%d/%d %d/%d/%d\n" % (a, 3 * i + 1, a, b, 3 * i + 2, b, c, 3 * i + 3, c)
                              for i, (a, b, c) in enumerate(f)))
    with open(stem + ".mtl", "w") as out:
        out.write("newmtl default\nKa 0.0 0.0 0.0\nmap_Kd %s_kd.png\nKs 0.0 0.0 0.0\n" % name)
    write_png_rgb(stem + "_kd.png", texture)


def read_obj_textured(path):
    """(vertices [V, 3] float32, faces [F, 3] int32 0-based, normals [V, 3] float32 or None, uv [F, 3, 2] float32, texture [H, W, 3]
    float32 in [0, 1]) of what write_obj_textured wrote: the texture is the `map_Kd` of the file that `mtllib` names."""
    import os

    from .texture import read_png_rgb
    v, n, vt, f, ft, mtl = [], [], [], [], [], None
    with open(path) as src:
        for line in src:
            parts = line.split()
            if not parts:
                continue
            if parts[0] == "mtllib":
                mtl = parts[1]
            elif parts[0] == "v":
                v.append([float(x) for x in parts[1:4]])
            elif parts[0] == "vn":
                n.append([float(x) for x in parts[1:4]])
            elif parts[0] == "vt":
                vt.append([float(x) for x in parts[1:3]])
            elif parts[0] == "f":
                f.append([int(x.split("/")[0]) - 1 for x in parts[1:4]])
                ft.append([int(x.split("/")[1]) - 1 for x in parts[1:4]])
    if mtl is None:
        raise ValueError("%s names no material library" % path)
    folder, image = os.path.dirname(os.path.abspath(path)), None
    with open(os.path.join(folder, mtl)) as src:
        for line in src:
            parts = line.split()
            if parts and parts[0] == "map_Kd":
                image = parts[1]
    if image is None:
        raise ValueError("%s has no map_Kd" % mtl)
    uv = np.asarray(vt, np.float32).reshape(-1, 2)[np.asarray(ft, np.int64).reshape(-1, 3)]
    texture = read_png_rgb(os.path.join(folder, image)).astype(np.float32) / 255
    return (np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int32).reshape(-1, 3),
            np.asarray(n, np.float32).reshape(-1, 3) if n else None, uv.reshape(-1, 3, 2), texture)
