"""Mesh cleaning and decimation without a GPU (csrc/mesh_clean.hip, gaussianip_amd/utils/mesh.py, tests/mesh_clean_reference.py): the
exported symbols and their NULL-pointer behaviour, the restatement against itself (union-find against a flood fill, the float32 grid
against exact rational arithmetic on dyadic inputs, the float32 and float64 keep decisions of the cleaning scene), and the argument
errors, which are raised before the library is touched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import mesh_clean_inputs as inputs
import mesh_clean_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_exported():
    from gaussianip_amd import _lib
    assert _lib.MESH_CLEAN_SYMBOLS == ["gip_mesh_components_rounds", "gip_mesh_component_stats", "gip_mesh_cluster_keys",
                                       "gip_mesh_cluster_count", "gip_mesh_cluster_place"]
    others = (_lib.RASTER_SYMBOLS + _lib.FIELD_SYMBOLS + _lib.SAMPLE_SYMBOLS + _lib.TEXTURE_SYMBOLS + _lib.MESH_SYMBOLS +
              _lib.MESH_GRAD_SYMBOLS)
    assert not set(_lib.MESH_CLEAN_SYMBOLS) & set(others)
    so = os.path.join(ROOT, "gaussianip_amd", "lib", "libgip_model.so")
    assert os.path.exists(so), "libgip_model.so is not built"
    names = {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout.splitlines()
             if ln.strip()}
    with open(os.path.join(ROOT, "include", "gip_model.h")) as fh:
        header = fh.read()
    lib = _lib.model_lib()
    for sym in _lib.MESH_CLEAN_SYMBOLS:
        assert sym in names, sym
        assert getattr(lib, sym) is not None
        assert "int %s(" % sym in header, sym
    assert "gs_renderer.py:346-350" in header


def test_null_pointers_are_refused():
    """Status 1 before anything is launched: no GPU is needed to get it."""
    from gaussianip_amd import _lib
    lib = _lib.model_lib()
    null = ctypes.c_void_p(None)
    assert lib.gip_mesh_components_rounds(null, 5, 7, null, null, 4, null) == 1
    assert lib.gip_mesh_component_stats(null, null, 5, 7, null, null, null, null) == 1
    assert lib.gip_mesh_cluster_keys(null, 7, 0.0, 0.0, 0.0, 0.5, 4, null, null) == 1
    assert lib.gip_mesh_cluster_count(null, 7, null, 5, 0.0, 0.0, 0.0, 0.5, 4, null, null) == 1
    assert lib.gip_mesh_cluster_place(null, 7, null, 5, null, 3, null, null, null, null, 0.0, 0.0, 0.0, 0.5, 4, 32, null, null) == 1
    # and the shapes outside the limits
    one = ctypes.c_void_p(8)            # never dereferenced: the shape is refused first
    assert lib.gip_mesh_components_rounds(one, 5, 7, one, one, 0, null) == 1
    assert lib.gip_mesh_cluster_keys(one, 7, 0.0, 0.0, 0.0, 0.5, 2049, one, null) == 1
    assert lib.gip_mesh_cluster_keys(one, 7, 0.0, 0.0, 0.0, 0.0, 4, one, null) == 1
    assert lib.gip_mesh_cluster_place(one, 7, one, 5, one, 3, one, one, one, one, 0.0, 0.0, 0.0, 0.5, 4, 48, one, null) == 1
    assert lib.gip_mesh_cluster_place(one, 7, one, 5, one, 8, one, one, one, one, 0.0, 0.0, 0.0, 0.5, 4, 32, one, null) == 1


def _meshes():
    out = [(f, len(v)) for v, f in (inputs.strips(F) for F in (1, 63, 64, 65, 257))]
    v, f, _ = inputs.mixed_components()
    out.append((f, len(v)))
    out += list(inputs.special().values())
    return out


def test_union_find_against_a_flood_fill():
    for faces, V in _meshes():
        got = ref.components(faces, V)
        assert np.array_equal(got, ref.flood_fill(faces, V))
        assert (got <= np.arange(V)).all() and (got[got] == got).all()
    sp = inputs.special()
    lab = ref.components(*sp["touching_blobs"])
    assert (lab[3:10] == 3).all() and (lab[10:] == 10).all() and (lab[:3] == np.arange(3)).all()      # two blobs share vertex 3: one component
    lab = ref.components(*sp["repeated_index"])
    assert lab[4] == 2 and lab[6] == 5 and lab[7] == 7
    assert len(np.unique(ref.components(*sp["three_faces_one_edge"]))) == 3          # the fan, the lone face and vertex 4
    v, f, owner = inputs.mixed_components()
    lab = ref.components(f, len(v))
    sizes = sorted(int((lab[f[:, 0]] == r).sum()) for r in np.unique(lab[f[:, 0]]))
    assert sizes == [1, 7, 8, 500] and len(np.unique(lab)) == 4 + 9


def test_float32_grid_against_rational_arithmetic():
    v, _ = inputs.dyadic_boundary()
    for n in (1, 2, 8, 16):
        idx, keys = ref.cell_indices(v, n)
        idx2, keys2 = ref.cell_indices_exact(v, n)
        assert np.array_equal(idx, idx2) and np.array_equal(keys, keys2)
    idx, _ = ref.cell_indices(v, 8)
    assert idx.min() == 0 and idx.max() == 7 and (idx[2:20, 0] == 7).all()         # the upper face of the box belongs to the last cell
    on_boundary = (np.round((v + 0.5) * 16).astype(int) % 2 == 0)
    assert on_boundary.mean() > 0.4 and np.array_equal(idx[on_boundary], np.minimum(np.round((v[on_boundary] + 0.5) * 8).astype(int), 7))


def test_clean_scene_is_decided_alike_in_both_precisions():
    """No component of the cleaning scene is within 1e-3 (relative) of either threshold, and the restatement keeps the same ones in
    float32 and in float64."""
    v, f, owner = inputs.clean_scene()
    a, b = ref.clean(v, f, dtype=np.float64), ref.clean(v, f, dtype=np.float32)
    assert a["num_components"] == b["num_components"] == 7 and a["num_kept"] == b["num_kept"] == 5
    for r in (a, b):
        for lab, sq in r["sq_diagonal"].items():
            assert abs(float(sq) / float(r["bar"]) - 1) > 1e-3
    for k in ("faces", "vertex_map", "face_map", "labels"):
        assert np.array_equal(a[k], b[k]), k
    kept = sorted(set(owner[a["face_map"]]))
    assert [inputs.CLEAN_PIECES[k] for k in kept] == ["sheet", "eight", "thin", "tie_a", "tie_b"]
    big = ref.clean(v, f, keep_largest=True)
    assert big["num_kept"] == 1 and set(owner[big["face_map"]]) == {0}
    tie = ref.clean(v, f, min_faces=0, min_diameter=0.0, keep_largest=True)
    assert tie["num_kept"] == 1


def test_restated_cluster_on_the_unit_cube():
    v, f = inputs.unit_cube()
    out = ref.cluster(v, f, 2048)
    assert np.array_equal(out["faces"], f) and np.array_equal(out["vertex_map"], np.arange(8)) and np.abs(out["vertices"] - v).max() < 1e-6
    assert ref.cluster(v, f, 1)["faces"].shape == (0, 3) and ref.face_count(v, f, 1) == 0 and ref.face_count(v, f, 2) == 12


def test_argument_errors_come_before_the_library():
    from gaussianip_amd import _lib
    from gaussianip_amd.utils import mesh
    before = dict(_lib.call_counts)
    v, f = torch.zeros((4, 3)), torch.zeros((2, 3), dtype=torch.int32)
    for call in (lambda: mesh.connected_components(f, 4), lambda: mesh.clean_mesh(v, f), lambda: mesh.cluster_decimate(v, f, 4),
                 lambda: mesh.decimate_mesh(v, f, 10), lambda: mesh.decimate_mesh(v, f, 0), lambda: mesh.cluster_face_count(v, f, 4),
                 lambda: mesh.connected_components(f.long(), 4), lambda: mesh.connected_components(torch.zeros((2, 4), dtype=torch.int32), 4),
                 lambda: mesh.clean_mesh(v.double(), f), lambda: mesh.cluster_decimate(torch.zeros((4, 2)), f, 4),
                 lambda: mesh.cluster_decimate(v.numpy(), f, 4)):
        with pytest.raises(ValueError):
            call()
    for grid in (0, 2049, -1, 2.5, True):
        with pytest.raises(ValueError):
            mesh._grid_arg("cluster_decimate", grid)
    assert mesh._grid_arg("cluster_decimate", 1) == 1 and mesh._grid_arg("cluster_decimate", 2048) == 2048
    assert dict(_lib.call_counts) == before


def test_settle_labels_and_null_pointers():
    """settle_labels over a fake propagation that needs k + 1 rounds (k that lower a label and the one that confirms) and whose flag stays
    raised until a call has run them: it returns after ceil((k + 1) / batch) calls and hands every call a zeroed flag.  A flag that never
    drops raises once the rounds pass limit + 1 + batch, the bound connected_components and unwrap_charts had.  _lib.ptr is null for
    None and for an empty tensor."""
    from gaussianip_amd import _lib
    from gaussianip_amd.utils.mesh import settle_labels
    limit = 10
    for batch in (1, 4, 8):
        for k in (0, 1, 3, 4, 7, 8, 9, 21):
            flag, seen = torch.zeros(1, dtype=torch.int32), []

            def step():
                seen.append(int(flag.item()))
                flag.fill_(1 if len(seen) * batch < k + 1 else 0)
                return flag
            assert settle_labels(step, 100, batch, "fake") is None
            assert len(seen) == -(-(k + 1) // batch) and not any(seen)
        calls = []

        def stuck():
            calls.append(None)
            return torch.ones(1, dtype=torch.int32)
        rounds = (limit + 1 + batch) // batch * batch + batch                            # the first whole batch past limit + 1 + batch
        with pytest.raises(RuntimeError, match=r"^fake labels did not settle in %d rounds$" % rounds):
            settle_labels(stuck, limit, batch, "fake labels")
        assert len(calls) * batch == rounds and rounds > limit + 1 + batch >= rounds - batch
    assert _lib.ptr(None).value is None and _lib.ptr(torch.empty(0)).value is None and _lib.ptr(torch.empty((0, 3))).value is None
    t = torch.zeros(2)
    assert _lib.ptr(t).value == t.data_ptr()
