"""The geometry terms of the mesh without a GPU (csrc/mesh_geom.hip, gaussianip_amd/utils/mesh_geometry.py): the exported symbols, the
entry points' argument checks (which launch nothing), MeshTopology on CPU tensors against a brute-force count in plain Python, the
inputs module against the fixture it was generated from, and the compiler's resource report of every kernel of the file."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import mesh_geometry_inputs as inputs
from test_model_no_spills_cpu import HIPCC, resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("mesh_geom_face_normals_kernel", "mesh_geom_normals_kernel",
           "mesh_geom_normalize_backward_kernel", "mesh_geom_normals_backward_kernel", "mesh_geom_laplacian_kernel",
           "mesh_geom_laplacian_backward_kernel", "mesh_geom_consistency_kernel", "mesh_geom_consistency_backward_kernel",
           "mesh_geom_finish_kernel")
STRIP = np.array([[0, 1, 2], [2, 1, 3], [3, 4, 2], [4, 3, 5], [1, 0, 6], [0, 1, 7]], np.int32)      # of test_edge_topology_against_a_count


def test_symbols_exported():
    from gaussianip_amd import _lib
    assert _lib.MESH_GEOM_SYMBOLS == ["gip_mesh_geometry_workspace_size", "gip_mesh_vertex_normals", "gip_mesh_vertex_normals_backward",
                                      "gip_mesh_laplacian_loss", "gip_mesh_laplacian_loss_backward", "gip_mesh_normal_consistency",
                                      "gip_mesh_normal_consistency_backward"]
    others = _lib.MESH_SYMBOLS + _lib.MESH_GRAD_SYMBOLS + _lib.MESH_MIP_SYMBOLS + _lib.MESH_CLEAN_SYMBOLS
    assert len(_lib.MESH_SYMBOLS) == 8 and not set(others) & set(_lib.MESH_GEOM_SYMBOLS)
    so = os.path.join(ROOT, "gaussianip_amd", "lib", "libgip_model.so")
    assert os.path.exists(so), "libgip_model.so is not built"
    names = {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout.splitlines()
             if ln.strip()}
    lib = _lib.model_lib()
    with open(os.path.join(ROOT, "include", "gip_model.h")) as fh:
        header = fh.read()
    for sym in _lib.MESH_GEOM_SYMBOLS:
        assert sym in names, sym
        assert getattr(lib, sym) is not None
        assert "int %s(" % sym in header, sym
    with open(os.path.join(ROOT, "gaussianip_amd", "csrc", "Makefile")) as fh:
        assert fh.read().count("mesh_geom.hip") == 2                 # a prerequisite of libgip_model.so and a source of its command
    from gaussianip_amd.utils import mesh_geometry
    assert mesh_geometry.__all__ == ["MeshTopology", "vertex_normals", "laplacian_loss", "normal_consistency", "Mesh"]
    for name in mesh_geometry.__all__:
        assert getattr(mesh_geometry, name) is not None


def test_argument_checks_launch_nothing():
    """Every check comes before the first launch, so these calls are safe on a machine without a GPU; `one` is a host address that a
    kernel would fault on."""
    from gaussianip_amd import _lib
    lib = _lib.model_lib()
    null = ctypes.c_void_p(None)
    buf = ctypes.create_string_buffer(64)
    one = ctypes.c_void_p(ctypes.addressof(buf))
    need = ctypes.c_size_t(77)
    assert lib.gip_mesh_geometry_workspace_size(1000, ctypes.byref(need)) == 0 and need.value == 4 * 4      # one float per 256 vertices
    assert lib.gip_mesh_geometry_workspace_size(256, ctypes.byref(need)) == 0 and need.value == 4
    assert lib.gip_mesh_geometry_workspace_size(0, ctypes.byref(need)) == 0 and need.value == 0
    assert lib.gip_mesh_geometry_workspace_size(-1, ctypes.byref(need)) == 1
    assert lib.gip_mesh_geometry_workspace_size(2 ** 31, ctypes.byref(need)) == 1
    assert lib.gip_mesh_geometry_workspace_size(5, None) == 1
    big_f = (2 ** 31 - 1) // 3 + 1
    # NULL pointers
    assert lib.gip_mesh_vertex_normals(null, null, null, null, 7, 5, null, null, null, null) == 1
    assert lib.gip_mesh_vertex_normals_backward(null, null, null, null, null, null, null, 7, 5, null, null, null) == 1
    assert lib.gip_mesh_laplacian_loss(null, null, null, 7, 5, null, null, null, 64, null) == 1
    assert lib.gip_mesh_laplacian_loss_backward(null, null, null, null, 7, 5, null, null) == 1
    assert lib.gip_mesh_normal_consistency(null, null, null, 7, 5, 3, null, null, 64, null) == 1
    assert lib.gip_mesh_normal_consistency_backward(null, null, null, null, 7, 5, 3, null, null) == 1
    # one NULL among dummies
    assert lib.gip_mesh_vertex_normals(one, one, one, one, 7, 5, one, one, null, null) == 1
    assert lib.gip_mesh_vertex_normals(one, one, one, one, 7, 5, null, one, one, null) == 1          # the per-face buffer is required
    assert lib.gip_mesh_vertex_normals_backward(one, one, one, one, one, one, one, 7, 5, null, one, null) == 1
    assert lib.gip_mesh_laplacian_loss(one, one, one, 7, 5, one, null, one, 64, null) == 1
    assert lib.gip_mesh_normal_consistency_backward(one, one, one, null, 7, 5, 3, one, null) == 1
    # sizes outside the limits, a short workspace
    assert lib.gip_mesh_vertex_normals(one, one, one, one, 7, big_f, one, one, one, null) == 1
    assert lib.gip_mesh_vertex_normals(one, one, one, one, 2 ** 31, 5, one, one, one, null) == 1
    assert lib.gip_mesh_vertex_normals(one, one, one, one, 7, -1, one, one, one, null) == 1
    assert lib.gip_mesh_vertex_normals_backward(one, one, one, one, one, one, one, -1, 5, one, one, null) == 1
    assert lib.gip_mesh_laplacian_loss(one, one, one, 7, 2 ** 31, one, one, one, 64, null) == 1
    assert lib.gip_mesh_laplacian_loss(one, one, one, 7, -1, one, one, one, 64, null) == 1
    assert lib.gip_mesh_laplacian_loss(one, one, one, 1000, 5, one, one, one, 15, null) == 1
    assert lib.gip_mesh_laplacian_loss_backward(one, one, one, one, 2 ** 31, 5, one, null) == 1
    assert lib.gip_mesh_normal_consistency(one, one, one, 1000, 5, 3, one, one, 15, null) == 1
    assert lib.gip_mesh_normal_consistency(one, one, one, 7, 5, -1, one, one, 64, null) == 1
    assert lib.gip_mesh_normal_consistency_backward(one, one, one, one, 7, 2 ** 31, 3, one, null) == 1
    # nothing to do: success, nothing launched or written
    assert lib.gip_mesh_vertex_normals(one, one, one, one, 7, 0, one, one, one, null) == 0
    assert lib.gip_mesh_vertex_normals(null, null, null, null, 0, 0, null, null, null, null) == 0
    assert lib.gip_mesh_vertex_normals_backward(one, one, one, one, one, one, one, 7, 0, one, one, null) == 0
    assert lib.gip_mesh_laplacian_loss(null, null, null, 0, 0, null, null, null, 0, null) == 0
    assert lib.gip_mesh_laplacian_loss_backward(null, null, null, null, 0, 0, null, null) == 0
    assert lib.gip_mesh_normal_consistency(one, one, one, 7, 0, 0, one, one, 64, null) == 0
    assert lib.gip_mesh_normal_consistency(null, null, null, 0, 0, 0, null, null, 0, null) == 0
    assert lib.gip_mesh_normal_consistency_backward(one, one, one, one, 7, 0, 0, one, null) == 0
    assert buf.raw == bytes(64)


def _count(tri, V):
    """(corners per vertex, neighbours per vertex, edges) of a face list, counted face by face."""
    corners, nbrs, edges = [[] for _ in range(V)], [set() for _ in range(V)], set()
    for f, face in enumerate(tri.tolist()):
        for k in range(3):
            corners[face[k]].append(3 * f + k)
            a, b = face[k], face[(k + 1) % 3]
            edges.add((min(a, b), max(a, b)))
            if a != b:
                nbrs[a].add(b)
                nbrs[b].add(a)
    return corners, [sorted(s) for s in nbrs], sorted(edges)


def _rows(start, items):
    start, items = start.tolist(), items.tolist()
    return [items[start[i]:start[i + 1]] for i in range(len(start) - 1)]


def _check_topology(topo, tri, V):
    corners, nbrs, edges = _count(tri, V)
    for t in (topo.faces, topo.corner_start, topo.corner_list, topo.nbr_start, topo.nbr_list):
        assert t.dtype == torch.int32 and t.is_contiguous() and not t.is_cuda
    assert np.array_equal(topo.faces.numpy(), tri) and topo.num_vertices == V and topo.num_faces == len(tri)
    assert topo.corner_start.shape == (V + 1,) and topo.corner_list.shape == (3 * len(tri),)
    assert _rows(topo.corner_start, topo.corner_list) == corners           # ascending inside a group: the count appends in order
    assert topo.nbr_start.shape == (V + 1,) and _rows(topo.nbr_start, topo.nbr_list) == nbrs
    assert topo.num_neighbours == sum(len(r) for r in nbrs) == int(topo.nbr_list.shape[0])
    assert topo.edges.dtype == torch.int64 and topo.edges.tolist() == [list(e) for e in edges]
    assert isinstance(topo.num_edges, int) and topo.num_edges == len(edges)
    return edges


def test_topology_against_a_count():
    from gaussianip_amd.utils.mesh_geometry import MeshTopology
    edges = _check_topology(MeshTopology(torch.from_numpy(STRIP), 8), STRIP, 8)
    assert len(edges) == 13 and (0, 1) in edges
    _check_topology(MeshTopology(torch.from_numpy(STRIP).long(), 11), STRIP, 11)         # int64 faces, vertices that no face names
    v, f, _, tags = inputs.mesh("a")
    V = v.shape[0]
    topo = MeshTopology(torch.from_numpy(f), V)
    edges = _check_topology(topo, f, V)
    gold = inputs.load_golden()
    assert np.array_equal(topo.edges.numpy(), gold["a_edges"]) and topo.num_edges == gold["a_edges"].shape[0] == 465
    a = tags["self_pair"][0]
    assert (a, a) in edges and sum(1 for e in edges if e[0] == e[1]) == 1           # E counts the self pair
    without = np.delete(f, tags["repeated_face"], 0)
    assert MeshTopology(torch.from_numpy(without), V).num_edges == topo.num_edges - 1
    rows = _rows(topo.nbr_start, topo.nbr_list)
    assert all(v_ not in rows[v_] for v_ in range(V))
    for i in (tags["isolated"],) + tags["unreferenced"]:
        assert rows[i] == [] and _rows(topo.corner_start, topo.corner_list)[i] == []
    assert tags["isolated"] in tags["unreferenced"] and len(tags["unreferenced"]) >= 1
    # mesh b: the fan's apex has 70 corners and 70 neighbours; its edges are the fixture's
    v, f, _, tags = inputs.mesh("b")
    topo = MeshTopology(torch.from_numpy(f), v.shape[0])
    assert np.array_equal(topo.edges.numpy(), gold["b_edges"])
    cs, ns = topo.corner_start.tolist(), topo.nbr_start.tolist()
    assert cs[tags["apex"] + 1] - cs[tags["apex"]] == 70 and ns[tags["apex"] + 1] - ns[tags["apex"]] == 70
    assert _rows(topo.nbr_start, topo.nbr_list)[tags["apex"]] == list(range(*tags["rim"]))


def test_topology_arguments():
    from gaussianip_amd.utils.mesh_geometry import MeshTopology
    tri = torch.from_numpy(STRIP)
    with pytest.raises(ValueError):
        MeshTopology(tri, 7)                                   # index 7 is out of range
    bad = tri.clone()
    bad[2, 1] = -1
    with pytest.raises(ValueError):
        MeshTopology(bad, 8)
    with pytest.raises(ValueError):
        MeshTopology(tri.float(), 8)
    with pytest.raises(ValueError):
        MeshTopology(tri.reshape(-1), 8)
    with pytest.raises(ValueError):
        MeshTopology(tri, 2 ** 31)
    empty = MeshTopology(torch.zeros((0, 3), dtype=torch.int64), 4)
    assert empty.num_edges == 0 and empty.num_neighbours == 0 and empty.num_faces == 0
    assert empty.faces.shape == (0, 3) and empty.corner_list.shape == (0,) and empty.nbr_list.shape == (0,) and empty.edges.shape == (0, 2)
    assert empty.corner_start.tolist() == [0] * 5 and empty.nbr_start.tolist() == [0] * 5
    assert MeshTopology(torch.zeros((0, 3), dtype=torch.int32), 0).corner_start.tolist() == [0]
    # its own copy of the faces
    mine = tri.clone()
    topo = MeshTopology(mine, 8)
    mine[0, 0] = 5
    assert np.array_equal(topo.faces.numpy(), STRIP)


def test_functions_refuse_what_is_not_a_gpu_tensor():
    from gaussianip_amd.utils import mesh_geometry as mg
    v, f, _, _ = inputs.mesh("a")
    topo = mg.MeshTopology(torch.from_numpy(f), v.shape[0])
    for fn in (mg.vertex_normals, mg.laplacian_loss, mg.normal_consistency):
        with pytest.raises(ValueError, match="float32 GPU tensor"):
            fn(torch.from_numpy(v), topo)
        with pytest.raises(ValueError, match="float32 GPU tensor"):
            fn(v, topo)
    mesh = mg.Mesh(torch.from_numpy(v), torch.from_numpy(f).long(), tag=3)
    mesh.add_extra("other", "x")
    assert mesh.extras == {"tag": 3, "other": "x"} and not mesh.requires_grad and mesh.v_rgb is None
    assert np.array_equal(mesh.edges.numpy(), inputs.load_golden()["a_edges"])          # the topology, lazily, on the CPU
    mesh.set_vertex_color(torch.zeros(v.shape[0], 3))
    assert mesh.v_rgb.shape == (v.shape[0], 3)
    for name, needle in (("v_tng", "atlas"), ("v_tex", "atlas"), ("t_tex_idx", "atlas")):
        with pytest.raises(NotImplementedError, match=needle):
            getattr(mesh, name)
    with pytest.raises(NotImplementedError, match="atlas"):
        mesh.unwrap_uv()
    with pytest.raises(NotImplementedError, match="clean_mesh"):
        mesh.remove_outlier(10)
    with pytest.raises(ValueError):
        mesh.v_nrm                                                                    # no CPU path for the terms


def test_inputs_reproduce_the_fixture():
    gold = inputs.load_golden()
    for name, (V, F) in (("a", (164, 305)), ("b", (2635, 5175))):
        v, f, w, tags = inputs.mesh(name)
        assert v.shape == (V, 3) and f.shape == (F, 3) and w.shape == (V, 3)
        for key, arr in (("v", v), ("f", f), ("w", w)):
            g = gold["%s_%s" % (name, key)]
            assert g.dtype == arr.dtype and g.shape == arr.shape and g.tobytes() == arr.tobytes(), (name, key)
        for q in inputs.QUANTITIES:
            assert gold["%s_%s" % (name, q)].dtype == np.float64 and float(gold["%s_err_%s" % (name, q)]) > 0
        assert np.isfinite(gold[name + "_g_nrm"]).all() and gold[name + "_v_nrm"].shape == (V, 3)
        for i in tags["unreferenced"]:
            assert np.array_equal(gold[name + "_v_nrm"][i], [0.0, 0.0, 1.0])
    assert os.path.getsize(inputs.GOLDEN) < 1024 * 1024


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_mesh_geom_kernels_do_not_spill(tmp_path):
    scratch, spilled, log = resource_usage("mesh_geom.hip", tmp_path / "o.o")
    for kernel in KERNELS:
        assert any(kernel in n for n in scratch), "no kernel-resource-usage remark for %s: %s" % (kernel, log[-500:])
    assert len(scratch) == len(KERNELS), sorted(scratch)
    bad = [(n, scratch[n], spilled.get(n, 0)) for n in scratch if scratch[n] or spilled.get(n, 0)]
    assert not bad, "kernels spilling: %s" % bad
