"""The field sampler without a GPU: the C-ABI's declarations, bindings, exports and host-side argument checks (csrc/field_sample.hip,
include/gip_model.h), and the mesh writers / readers of gaussianip_amd/utils/mesh.py with per-vertex colours and normals."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

V = np.array([[0, 0, 0], [1, 0.5, 0], [0, 1, 1 / 3], [-2.5e-7, 3, 1e10]], np.float32)
F = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
C = np.array([[0.2, 0.5, 0.8], [0, 1, 0.333], [1, 1, 1], [0.0019, 0.998, 0.5]], np.float32)
N = np.array([[0, 0, 1], [0, -1, 0], [0.6, 0.8, 0], [0, 0, 0]], np.float32)


def test_symbols_declared_bound_and_exported():
    from gaussianip_amd import _lib
    header = open(os.path.join(ROOT, "include", "gip_model.h")).read()
    assert _lib.SAMPLE_SYMBOLS == ["gip_field_sample_workspace_size", "gip_field_sample"]
    lib = ctypes.CDLL(os.path.join(_lib.LIB_DIR, "libgip_model.so"))
    for sym in _lib.SAMPLE_SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, header), sym
        getattr(lib, sym)
    bound = _lib.model_lib()
    need, field_need = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert bound.gip_field_sample_workspace_size(1000, 128, 16, ctypes.byref(need)) == 0 and need.value == 1000 * 48
    assert bound.gip_field_workspace_size(1000, 128, 16, ctypes.byref(field_need)) == 0 and field_need.value == need.value
    assert bound.gip_field_sample_workspace_size(1000, 30, 16, ctypes.byref(need)) == 1      # num_blocks does not divide the resolution
    assert bound.gip_field_sample_workspace_size(-1, 32, 8, ctypes.byref(need)) == 1
    assert bound.gip_field_sample_workspace_size(10, 2048, 2048, ctypes.byref(need)) == 1    # more than 1024 blocks per axis
    assert bound.gip_field_sample_workspace_size(10, 32, 8, None) == 1


def test_host_side_argument_checks_launch_nothing():
    from gaussianip_amd import _lib
    bound = _lib.model_lib()

    def call(P, R, nb, V_, color_sum=None, rgb=None):
        return bound.gip_field_sample(None, None, None, None, rgb, P, None, 1.0, None, R, nb, 0.375, None, None, V_, None, 0, None, None,
                                      color_sum, None)
    assert call(0, 32, 8, 0) == 0                    # no points: a successful no-op
    assert call(0, 30, 16, 0) == 1                           # shape outside the limits
    assert call(0, 32, 8, 2 ** 31) == 1                      # more points than an int32 counts
    assert call(0, 32, 8, -1) == 1
    assert call(0, 32, 8, 10) == 1                           # points without their arrays
    assert call(5, 32, 8, 0, color_sum=ctypes.c_void_p(16)) == 1      # a colour output without colours (nothing is dereferenced)


def test_plain_obj_is_unchanged(tmp_path):
    from gaussianip_amd.utils.mesh import read_obj, write_obj
    path = str(tmp_path / "plain.obj")
    write_obj(path, V, F)
    text = open(path).read()
    assert text == ("# 4 vertices, 2 faces\nv 0 0 0\nv 1 0.5 0\nv 0 1 0.333333343\nv -2.49999999e-07 3 1e+10\n"
                    "f 1 2 3\nf 3 2 4\n")
    rv, rf = read_obj(path)
    assert np.array_equal(rv, V) and np.array_equal(rf, F) and rf.dtype == np.int32


@pytest.mark.parametrize("with_colors,with_normals", [(True, True), (True, False), (False, True)])
def test_obj_round_trip(tmp_path, with_colors, with_normals):
    from gaussianip_amd.utils.mesh import read_obj, read_obj_full, write_obj
    path = str(tmp_path / "mesh.obj")
    write_obj(path, V, F, colors=C if with_colors else None, normals=N if with_normals else None)
    lines = open(path).read().splitlines()
    assert sum(ln.startswith("vn ") for ln in lines) == (len(V) if with_normals else 0)
    assert all(len(ln.split()) == (7 if with_colors else 4) for ln in lines if ln.startswith("v "))
    assert ("f 1//1 2//2 3//3" in lines) == with_normals and ("f 1 2 3" in lines) == (not with_normals)
    rv, rf, rc, rn = read_obj_full(path)
    assert np.array_equal(rv, V) and np.array_equal(rf, F)
    assert np.array_equal(rc, C) if with_colors else rc is None
    assert np.array_equal(rn, N) if with_normals else rn is None
    pv, pf = read_obj(path)                                  # the two-value reader still reads such a file
    assert np.array_equal(pv, V) and np.array_equal(pf, F)


@pytest.mark.parametrize("with_colors,with_normals", [(True, True), (True, False), (False, True), (False, False)])
def test_ply_round_trip(tmp_path, with_colors, with_normals):
    from gaussianip_amd.utils.mesh import read_ply_mesh, write_ply_mesh
    path = str(tmp_path / "mesh.ply")
    write_ply_mesh(path, V, F, colors=C if with_colors else None, normals=N if with_normals else None)
    raw = open(path, "rb").read()
    header = raw[:raw.index(b"end_header\n")].decode("ascii").splitlines()
    assert header[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 4"]
    props = [ln for ln in header if ln.startswith("property")]
    want = ["property float x", "property float y", "property float z"]
    want += ["property float nx", "property float ny", "property float nz"] if with_normals else []
    want += ["property uchar red", "property uchar green", "property uchar blue"] if with_colors else []
    assert props == want + ["property list uchar int vertex_indices"]
    stride = 12 + (12 if with_normals else 0) + (3 if with_colors else 0)
    assert len(raw) == raw.index(b"end_header\n") + len(b"end_header\n") + 4 * stride + 2 * 13
    rv, rf, rc, rn = read_ply_mesh(path)
    assert np.array_equal(rv, V) and np.array_equal(rf, F) and rf.dtype == np.int32
    if with_colors:
        assert rc.dtype == np.float32 and np.abs(rc - C).max() <= 0.5 / 255 + 1e-7      # within the 1/255 of the quantisation
    else:
        assert rc is None
    assert np.array_equal(rn, N) if with_normals else rn is None


def test_empty_mesh_round_trips(tmp_path):
    from gaussianip_amd.utils.mesh import read_obj_full, read_ply_mesh, write_obj, write_ply_mesh
    e3, ei = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    write_obj(str(tmp_path / "e.obj"), e3, ei, colors=e3, normals=e3)
    write_ply_mesh(str(tmp_path / "e.ply"), e3, ei, colors=e3, normals=e3)
    rv, rf, _, _ = read_obj_full(str(tmp_path / "e.obj"))
    assert rv.shape == (0, 3) and rf.shape == (0, 3)
    rv, rf, rc, rn = read_ply_mesh(str(tmp_path / "e.ply"))
    assert rv.shape == (0, 3) and rf.shape == (0, 3) and rc.shape == (0, 3) and rn.shape == (0, 3)


def test_sample_fields_rejects_indivisible_resolution():
    import torch
    from gaussianip_amd.scene import GaussianModel
    with pytest.raises(ValueError, match="divide"):
        GaussianModel(0, device="cpu").sample_fields(torch.zeros(4, 3), resolution=30, num_blocks=16)
    with pytest.raises(RuntimeError, match="GPU"):
        GaussianModel(0, device="cpu").sample_fields(torch.zeros(4, 3), resolution=32, num_blocks=8)
