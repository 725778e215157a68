"""The tetrahedral SDF grid without a GPU (csrc/mesh_tets.hip, gaussianip_amd/utils/isosurface.py): the inputs module and the torch
restatement against the fixture they were generated with, TetGrid's tables on CPU tensors, the Kuhn grid, the entry points' argument
checks (which launch nothing), and the compiler's resource report of every kernel of the file."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import isosurface_inputs as inputs
import isosurface_reference as reference
from test_model_no_spills_cpu import HIPCC, resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("tet_mark_kernel", "tet_emit_kernel", "tet_backward_kernel", "tet_sdf_diff_kernel", "tet_sdf_diff_finish_kernel",
           "tet_sdf_diff_backward_kernel")


def _grid32():
    from gaussianip_amd.utils.isosurface import TetGrid
    v, t = inputs.grid()
    return TetGrid(torch.from_numpy(v), torch.from_numpy(t))


def test_symbols_exported():
    from gaussianip_amd import _lib
    from gaussianip_amd.utils import isosurface
    so = os.path.join(ROOT, "gaussianip_amd", "lib", "libgip_model.so")
    assert os.path.exists(so), "libgip_model.so is not built"
    names = {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout.splitlines()
             if ln.strip()}
    lib = _lib.model_lib()
    with open(os.path.join(ROOT, "include", "gip_model.h")) as fh:
        header = fh.read()
    assert len(_lib.MESH_TET_SYMBOLS) == 6
    for sym in _lib.MESH_TET_SYMBOLS:
        assert sym in names and getattr(lib, sym) is not None and "int %s(" % sym in header, sym
    with open(os.path.join(ROOT, "gaussianip_amd", "csrc", "Makefile")) as fh:
        assert fh.read().count("mesh_tets.hip") == 2                 # a prerequisite of libgip_model.so and a source of its command
    assert isosurface.__all__ == ["TetGrid", "marching_tetrahedra", "tet_sdf_diff", "MarchingTetrahedraHelper", "TetrahedraSDFGrid",
                                  "scale_tensor"]
    from gaussianip_amd.scene import GaussianModel
    assert callable(GaussianModel.to_tetrahedra_sdf_grid)


def test_inputs_reproduce_the_fixture():
    gold = inputs.load_golden()
    v, t = inputs.grid()
    assert v.shape == (5034, 3) and v.dtype == np.float32 and t.shape == (24444, 4)
    for name in inputs.CASES:
        sdf, deformation = inputs.case(name)
        assert sdf.shape == (5034, 1) and sdf.dtype == np.float32 and gold[name + "_sdf"].tobytes() == sdf.tobytes(), name
        assert (deformation is None) == (name + "_def" not in gold)
        if deformation is not None:
            assert gold[name + "_def"].dtype == np.float32 and gold[name + "_def"].tobytes() == deformation.tobytes()
        w = inputs.weights(name, gold[name + "_v_pos"].shape[0])
        assert gold[name + "_w"].tobytes() == w.tobytes() and gold[name + "_w"].shape == w.shape
        for q in inputs.QUANTITIES[name]:
            assert gold["%s_%s" % (name, q)].dtype == np.float64 and float(gold["%s_err_%s" % (name, q)]) > 0, (name, q)
    # every marching-tetrahedra case occurs often on the noise input, and the magnitude's floor holds
    sdf, _ = inputs.case("noise")
    assert inputs.case_histogram(sdf, t).min() >= inputs.MIN_CASE_COUNT and np.abs(sdf).min() >= 0.25
    sdf, _ = inputs.case("zeros")
    assert 400 < int((sdf == 0).sum()) < 600
    assert os.path.getsize(inputs.GOLDEN) <= 1000 * 1000


def _restated(name, dtype):
    """The quantities of the fixture from the restatement, on the CPU in `dtype`."""
    v, t = inputs.grid()
    sdf, deformation = inputs.case(name)
    tets = torch.from_numpy(t)
    s = torch.from_numpy(sdf).to(dtype).requires_grad_(True)
    pos = torch.from_numpy(v).to(dtype).requires_grad_(True)
    if deformation is not None:
        leaf = torch.from_numpy(deformation).to(dtype).requires_grad_(True)
        grid_vertices = pos + reference.normalize_grid_deformation(leaf, inputs.RESOLUTION)
    else:
        leaf, grid_vertices = pos, pos
    v_pos, faces = reference.marching_tetrahedra(grid_vertices, s, tets)
    w = torch.from_numpy(inputs.weights(name, v_pos.shape[0])).to(dtype)
    g_sdf, g_leaf = torch.autograd.grad((w * v_pos).sum(), (s, leaf))
    out = {"v_pos": v_pos.detach(), "faces": faces, "g_sdf": g_sdf, "g_def" if deformation is not None else "g_pos": g_leaf}
    s = torch.from_numpy(sdf).to(dtype).requires_grad_(True)
    val = reference.tet_sdf_diff(s, reference.all_edges(tets))
    out["tsd"], (out["g_tsd"],) = val.detach(), torch.autograd.grad(val, s)
    return out


@pytest.mark.parametrize("name", inputs.CASES)
def test_restatement_against_the_fixture(name):
    gold = inputs.load_golden()
    got = _restated(name, torch.float64)
    assert np.array_equal(got["faces"].numpy(), gold[name + "_faces"])
    for q in inputs.QUANTITIES[name]:
        ref = gold["%s_%s" % (name, q)]
        assert got[q].dtype == torch.float64 and got[q].shape == ref.shape
        assert np.abs(got[q].numpy() - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (name, q)
    # in float32 the restated vertex formula gives the bits of the reference's float32 run: its error against float64 is the fixture's
    got32 = _restated(name, torch.float32)
    assert np.array_equal(got32["faces"].numpy(), gold[name + "_faces"])
    assert float(np.abs(got32["v_pos"].double().numpy() - gold[name + "_v_pos"]).max()) == float(gold[name + "_err_v_pos"])


def test_tet_grid_tables():
    gold = inputs.load_golden()
    grid = _grid32()
    v, t = inputs.grid()
    Nv, Ft, Ne = 5034, 24444, gold["all_edges"].shape[0]
    assert (grid.num_vertices, grid.num_tets, grid.num_edges) == (Nv, Ft, Ne)
    assert grid.vertices.dtype == torch.float32 and grid.indices.dtype == torch.int32 and grid.edges.dtype == torch.int64
    for name in ("edges32", "tet_edge_ids", "vert_edge_start", "vert_edge_list", "indices"):
        x = getattr(grid, name)
        assert x.dtype == torch.int32 and x.is_contiguous(), name
    assert np.array_equal(grid.edges.numpy(), gold["all_edges"]) and np.array_equal(grid.edges32.numpy(), gold["all_edges"])
    assert np.array_equal(reference.all_edges(torch.from_numpy(t)).numpy(), gold["all_edges"])
    e = grid.edges.numpy()
    assert (e[:, 0] < e[:, 1]).all()
    key = e[:, 0] * Nv + e[:, 1]
    assert (np.diff(key) > 0).all()                                       # sorted and unique
    # tet_edge_ids round-trips to the tetrahedra's corner pairs, in the reference's pair order
    pairs = t[:, [0, 1, 0, 2, 0, 3, 1, 2, 1, 3, 2, 3]].reshape(Ft, 6, 2)
    ids = grid.tet_edge_ids.numpy()
    assert ids.shape == (Ft, 6) and ids.min() == 0 and ids.max() == Ne - 1
    assert np.array_equal(e[ids], np.sort(pairs, 2))
    # the rows: complete (every end of every edge once, with the right end bit) and ascending
    start, items = grid.vert_edge_start.numpy().astype(np.int64), grid.vert_edge_list.numpy().astype(np.int64)
    assert start.shape == (Nv + 1,) and start[0] == 0 and start[-1] == 2 * Ne == items.shape[0] and (np.diff(start) >= 0).all()
    owner = np.repeat(np.arange(Nv), np.diff(start))
    assert np.array_equal(e[items >> 1, items & 1], owner)
    assert np.array_equal(np.sort(items), np.arange(2 * Ne))
    same_row = owner[1:] == owner[:-1]
    assert (np.diff(items)[same_row] > 0).all()
    assert np.diff(start).max() < 64                                     # no row of this grid is longer than a wave


def test_kuhn_grid():
    from gaussianip_amd.utils.isosurface import TetGrid
    grid = TetGrid.kuhn(2)
    assert grid.num_vertices == 27 and grid.num_tets == 48 and grid.num_edges == 98
    v, t = grid.vertices.double().numpy(), grid.indices.numpy().astype(np.int64)
    assert v.min() == 0.0 and v.max() == 1.0 and np.array_equal(v[(1 * 3 + 2) * 3 + 0], [0.5, 1.0, 0.0])
    a, b, c, d = (v[t[:, k]] for k in range(4))
    det = np.einsum("ij,ij->i", np.cross(b - a, c - a), d - a)
    assert (det > 0).all() and abs(det.sum() / 6.0 - 1.0) < 1e-12        # positively oriented, and they fill the cube
    faces = np.sort(t[:, [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]].reshape(-1, 3), 1)
    uniq, count = np.unique(faces, axis=0, return_counts=True)
    on_boundary = np.array([(v[f][:, ax] == side).all() for f in uniq for ax in range(3) for side in (0.0, 1.0)]).reshape(-1, 6).any(1)
    assert np.array_equal(count[on_boundary], np.ones(on_boundary.sum(), np.int64)) and on_boundary.sum() == 6 * 2 * 4
    assert np.array_equal(count[~on_boundary], np.full((~on_boundary).sum(), 2))        # every interior face: exactly two tetrahedra
    # the orientation the reference's own grid has, which is what winds the table's faces outward
    v32, t32 = inputs.grid()
    a, b, c, d = (v32.astype(np.float64)[t32[:, k]] for k in range(4))
    assert (np.einsum("ij,ij->i", np.cross(b - a, c - a), d - a) > 0).all()
    # a sphere inside the Kuhn grid at R = 8, through the restatement: closed, and wound outward for a distance negative inside
    grid = TetGrid.kuhn(8)
    sdf = (grid.vertices.double() - 0.5).norm(dim=1) - 0.3
    vp, f = reference.marching_tetrahedra(grid.vertices.double(), sdf, grid.indices)
    p = vp[f]
    volume = float((torch.cross(p[:, 0], p[:, 1], dim=1) * p[:, 2]).sum() / 6.0)
    assert 0.5 * (4.0 / 3.0 * np.pi * 0.3 ** 3) < volume < 4.0 / 3.0 * np.pi * 0.3 ** 3
    with pytest.raises(ValueError):
        TetGrid.kuhn(0)


def test_tet_grid_arguments(tmp_path):
    from gaussianip_amd.utils.isosurface import TetGrid, marching_tetrahedra, tet_sdf_diff
    v = torch.rand(5, 3)
    t = torch.tensor([[0, 1, 2, 3], [1, 2, 3, 4]])
    grid = TetGrid(v.double(), t.int())                                 # float64 vertices and int32 indices are converted
    assert grid.vertices.dtype == torch.float32 and grid.num_edges == 9 and grid.edges.tolist()[0] == [0, 1]
    bad = t.clone()
    bad[1, 2] = 5
    with pytest.raises(ValueError, match=r"\[0, 5\)"):
        TetGrid(v, bad)
    bad[1, 2] = -1
    with pytest.raises(ValueError):
        TetGrid(v, bad)
    for wrong in ((v[:, :2], t), (v, t[:, :3]), (v, t.float()), (v.long(), t)):
        with pytest.raises(ValueError):
            TetGrid(*wrong)
    mine = t.clone()
    grid = TetGrid(v, mine)
    mine[0, 0] = 4
    assert grid.indices.tolist() == t.tolist()                          # its own copy
    empty = TetGrid(v, torch.zeros((0, 4), dtype=torch.int64))
    assert empty.num_edges == 0 and empty.vert_edge_start.tolist() == [0] * 6 and empty.tet_edge_ids.shape == (0, 6)
    path = str(tmp_path / "grid.npz")
    np.savez(path, vertices=v.double().numpy(), indices=t.numpy())
    loaded = TetGrid.from_npz(path)
    assert torch.equal(loaded.vertices, v) and torch.equal(loaded.edges, grid.edges) and loaded.to("cpu") is loaded
    # the kernels have no CPU path
    for fn in (lambda: marching_tetrahedra(grid, torch.zeros(5)), lambda: tet_sdf_diff(torch.zeros(5, 1), grid)):
        with pytest.raises(ValueError, match="float32 GPU tensor"):
            fn()


def test_argument_checks_launch_nothing():
    """Every check comes before the first launch, so these calls are safe on a machine without a GPU; `one` is a host address that a
    kernel would fault on."""
    from gaussianip_amd import _lib
    lib = _lib.model_lib()
    null = ctypes.c_void_p(None)
    buf = ctypes.create_string_buffer(64)
    one = ctypes.c_void_p(ctypes.addressof(buf))
    need = ctypes.c_size_t(77)
    assert lib.gip_tet_workspace_size(1000, ctypes.byref(need)) == 0 and need.value == 4 * 8      # a float and a count per 256 edges
    assert lib.gip_tet_workspace_size(0, ctypes.byref(need)) == 0 and need.value == 0
    assert lib.gip_tet_workspace_size(-1, ctypes.byref(need)) == 1 and lib.gip_tet_workspace_size(5, None) == 1
    big = 2 ** 31
    # NULL pointers
    assert lib.gip_tet_mark(null, null, null, 7, 5, 3, null, null) == 1
    assert lib.gip_tet_mark(one, one, one, 7, 5, 3, null, null) == 1
    assert lib.gip_tet_emit(null, null, null, null, null, null, null, 7, 5, 3, 2, 1, 1, null, null, null, null) == 1
    assert lib.gip_tet_emit(one, one, one, one, one, one, one, 7, 5, 3, 2, 1, 1, one, null, one, null) == 1
    assert lib.gip_tet_emit(one, one, one, one, one, one, one, 7, 5, 3, 2, 1, 1, one, one, null, null) == 1
    assert lib.gip_tet_backward(one, one, one, one, one, one, one, 7, 5, 2, one, null, null) == 1
    assert lib.gip_tet_backward(one, one, one, one, one, one, null, 7, 5, 2, null, one, null) == 1
    assert lib.gip_tet_sdf_diff(one, one, 7, 5, one, null, one, 64, null) == 1
    assert lib.gip_tet_sdf_diff_backward(one, one, one, one, null, one, 7, 5, one, null) == 1
    # sizes outside the limits, totals that do not fit the grid, a short workspace
    assert lib.gip_tet_mark(one, one, one, big, 5, 3, one, null) == 1
    assert lib.gip_tet_mark(one, one, one, 7, big // 2, 3, one, null) == 1
    assert lib.gip_tet_mark(one, one, one, 7, 5, big // 6 + 1, one, null) == 1
    assert lib.gip_tet_mark(one, one, one, 7, -1, 3, one, null) == 1
    assert lib.gip_tet_mark(one, one, one, 0, 5, 3, one, null) == 1
    assert lib.gip_tet_emit(one, one, one, one, one, one, one, 7, 5, 3, 6, 1, 1, one, one, one, null) == 1       # more vertices than edges
    assert lib.gip_tet_emit(one, one, one, one, one, one, one, 7, 5, 3, 2, 3, 1, one, one, one, null) == 1       # more than Ft tetrahedra
    assert lib.gip_tet_emit(one, one, one, one, one, one, one, 7, 5, 3, 0, 1, 0, one, one, one, null) == 1       # faces without vertices
    assert lib.gip_tet_backward(one, one, one, one, one, one, one, 7, 5, 6, one, one, null) == 1
    assert lib.gip_tet_sdf_diff(one, one, 7, 1000, one, one, one, 31, null) == 1
    # nothing to do: success, nothing launched or written
    assert lib.gip_tet_mark(one, null, null, 7, 0, 0, one, null) == 0
    assert lib.gip_tet_emit(one, one, null, null, null, null, null, 7, 0, 0, 0, 0, 0, null, null, null, null) == 0
    assert lib.gip_tet_backward(null, null, null, null, null, null, null, 0, 0, 0, null, null, null) == 0
    assert lib.gip_tet_sdf_diff(one, null, 7, 0, one, one, null, 0, null) == 0
    assert lib.gip_tet_sdf_diff_backward(null, null, null, null, null, null, 0, 0, null, null) == 0
    assert buf.raw == bytes(64)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_mesh_tets_kernels_do_not_spill(tmp_path):
    scratch, spilled, log = resource_usage("mesh_tets.hip", tmp_path / "o.o")
    for kernel in KERNELS:
        assert any(kernel in n for n in scratch), "no kernel-resource-usage remark for %s: %s" % (kernel, log[-500:])
    assert len(scratch) == len(KERNELS), sorted(scratch)
    bad = [(n, scratch[n], spilled.get(n, 0)) for n in scratch if scratch[n] or spilled.get(n, 0)]
    assert not bad, "kernels spilling: %s" % bad
