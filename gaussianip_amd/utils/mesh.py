"""Iso-surface of a regular grid as an indexed triangle mesh (csrc/field.hip: marching tetrahedra on the Kuhn decomposition;
include/gip_model.h gip_surface_count / gip_surface_emit), and a Wavefront OBJ writer / reader for it.

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


def write_obj(path, vertices, faces):
    """Wavefront OBJ: `v x y z` lines (9 significant digits: a float32 survives the round trip), `f a b c` lines, 1-based."""
    v = np.asarray(vertices.detach().cpu() if isinstance(vertices, torch.Tensor) else vertices, dtype=np.float32)
    f = np.asarray(faces.detach().cpu() if isinstance(faces, torch.Tensor) else faces, dtype=np.int64) + 1
    with open(path, "w") as out:
        out.write("# %d vertices, %d faces\n" % (v.shape[0], f.shape[0]))
        out.write("".join("v %.9g %.9g %.9g\n" % (float(a), float(b), float(c)) for a, b, c in v))
        out.write("".join("f %d %d %d\n" % (a, b, c) for a, b, c in f))


def read_obj(path):
    """(vertices [V, 3] float32, faces [F, 3] int32, 0-based) of an OBJ that write_obj wrote (v and triangular f lines only)."""
    v, f = [], []
    with open(path) as src:
        for line in src:
            parts = line.split()
            if not parts:
                continue
            if parts[0] == "v":
                v.append([float(x) for x in parts[1:4]])
            elif parts[0] == "f":
                f.append([int(x.split("/")[0]) - 1 for x in parts[1:4]])
    return np.asarray(v, np.float32).reshape(-1, 3), np.asarray(f, np.int32).reshape(-1, 3)
