"""Cleaning and decimating the extracted mesh on the GPU (csrc/mesh_clean.hip; connected_components, clean_mesh, cluster_decimate,
decimate_mesh of gaussianip_amd/utils/mesh.py; the clean / decimate_target keywords of GaussianModel's mesh methods).

Everything discrete (labels, kept components, maps, cell membership, faces) is compared exactly with tests/mesh_clean_reference.py.
Positions of the clustering are measured against the restatement in float64; the bar is 8 times the float32 restatement's own maximum
error against float64 on the same input: the kernel adds in another order than numpy, and the solve amplifies either by at most
1 / lambda + 1.  The cube's bar, 3 l / (1 + 3 l) sqrt(3) h, is not measured but derived: in a corner cell the quadric is diagonal with
equal weights w = tr / 3 per axis (the tessellation and the grid share the corner's symmetry), so per axis
x - d = l tr (m - d) / (w + l tr) = 3 l / (1 + 3 l) (m - d) with |m - d| <= 1 cell.

With GIP_MESH_CLEAN_PARITY_OUT=<file> the figures are written there as JSON (profiles/mesh_clean_parity.json is such a run)."""
import functools
import json
import math
import os

import numpy as np
import pytest
import torch

import field_inputs
import mesh_clean_inputs as inputs
import mesh_clean_reference as ref
import sample_inputs
import scenes

pytestmark = pytest.mark.gpu
FACTOR = 8.0
_figures = {}


@pytest.fixture(scope="module", autouse=True)
def _write_figures():
    yield
    out = os.environ.get("GIP_MESH_CLEAN_PARITY_OUT")
    if out and _figures:
        with open(out, "w") as f:
            f.write(json.dumps(_figures, indent=1, sort_keys=True) + "\n")


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _model(cl, colors=None):
    from gaussianip_amd.scene import GaussianModel
    from gaussianip_amd.utils.sh import C0
    gm = GaussianModel(0)
    gm._xyz, gm._opacity = _cu(cl["xyz"]), _cu(cl["opacity"])
    gm._scaling, gm._rotation = _cu(cl["scaling"]), _cu(cl["rotation"])
    P = cl["xyz"].shape[0]
    rgb = np.full((P, 3), 0.5, np.float32) if colors is None else colors
    gm._features_dc = ((_cu(rgb) - 0.5) / C0).reshape(P, 1, 3).contiguous()
    gm._features_rest = torch.zeros((P, 0, 3), device="cuda")
    return gm


# ---------------------------------------------------------------------------------------------------------------- 1. components
def _labels(faces, V):
    from gaussianip_amd.utils.mesh import connected_components
    got = connected_components(_cu(np.asarray(faces, np.int32).reshape(-1, 3)), V)
    assert got.dtype == torch.int32 and got.shape == (V,) and got.is_cuda
    return _np(got)


def test_components_of_a_permuted_strip():
    """4096 vertices in one strip with shuffled indices: the minimum travels through many rounds, and the loop ends."""
    from gaussianip_amd import _lib
    v, f = inputs.permuted_strip()
    before = _lib.call_counts.get("gip_mesh_components_rounds", 0)
    got = _labels(f, len(v))
    batches = _lib.call_counts.get("gip_mesh_components_rounds", 0) - before
    print("permuted strip of %d vertices: %d batches of rounds" % (len(v), batches))
    assert not got.any() and np.array_equal(got, ref.components(f, len(v)))
    assert 2 <= batches <= (len(v) + 1) // 4 + 2


@pytest.mark.parametrize("F", [1, 63, 64, 65, 257])
def test_components_face_counts(F):
    v, f = inputs.strips(F)
    assert len(f) == F
    assert np.array_equal(_labels(f, len(v)), ref.components(f, len(v)))


def test_components_mixed_and_special():
    v, f, _ = inputs.mixed_components()
    want = ref.components(f, len(v))
    assert len(np.unique(want)) == 4 + 9                       # four pieces and nine unreferenced vertices
    assert np.array_equal(_labels(f, len(v)), want)
    for name, (faces, V) in inputs.special().items():
        assert np.array_equal(_labels(faces, V), ref.components(faces, V)), name
    assert np.array_equal(_labels(np.zeros((0, 3), np.int32), 0), np.zeros(0, np.int32))
    bad = np.array([[0, 1, 2], [3, 4, 99], [-1, 5, 6], [2, 7, 8]], np.int32)         # faces with an index out of range are ignored
    assert np.array_equal(_labels(bad, 9), ref.components(bad, 9))
    a, b = _labels(f, len(v)), _labels(f[::-1].copy(), len(v))                         # nothing but the set of faces matters
    assert np.array_equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- 2. clean_mesh
def _clean(v, f, **kw):
    from gaussianip_amd.utils.mesh import clean_mesh
    return clean_mesh(_cu(v), _cu(f), **kw)


def _same_clean(got, want):
    gv, gf, info = got
    assert gv.dtype == torch.float32 and gf.dtype == torch.int32 and info["vertex_map"].dtype == torch.int32 and info["face_map"].dtype == torch.int32
    assert np.array_equal(_np(gv), want["vertices"]) and np.array_equal(_np(gf), want["faces"])
    for k in ("labels", "vertex_map", "face_map"):
        assert np.array_equal(_np(info[k]), want[k]), k
    assert info["num_components"] == want["num_components"] and info["num_kept"] == want["num_kept"]


def test_clean_mesh_against_the_restatement():
    v, f, owner = inputs.clean_scene()
    got = _clean(v, f)
    _same_clean(got, ref.clean(v, f))
    kept = {inputs.CLEAN_PIECES[k] for k in owner[_np(got[2]["face_map"])]}
    assert kept == {"sheet", "eight", "thin", "tie_a", "tie_b"}             # seven faces go, eight stay; thin stays, tiny goes
    assert got[2]["num_components"] == 7 and got[2]["num_kept"] == 5
    _same_clean(_clean(v, f, min_faces=9), ref.clean(v, f, min_faces=9))
    _same_clean(_clean(v, f, min_faces=0, min_diameter=0.0), ref.clean(v, f, min_faces=0, min_diameter=0.0))
    _same_clean(_clean(v, f, min_diameter=0.2), ref.clean(v, f, min_diameter=0.2))
    again = _clean(v, f)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])
    assert all(torch.equal(got[2][k], again[2][k]) for k in ("labels", "vertex_map", "face_map"))
    # the kept faces are the input's, in its order, on the input's vertices
    fm, vm = _np(got[2]["face_map"]), _np(got[2]["vertex_map"])
    assert (np.diff(fm) > 0).all() and np.array_equal(_np(got[0])[_np(got[1])], v[f[fm]])
    assert np.array_equal(np.nonzero(vm >= 0)[0][vm[vm >= 0]], np.nonzero(vm >= 0)[0]) and (np.diff(vm[vm >= 0]) == 1).all()


def test_clean_mesh_keep_largest_and_its_tie():
    v, f, owner = inputs.clean_scene()
    got = _clean(v, f, keep_largest=True)
    _same_clean(got, ref.clean(v, f, keep_largest=True))
    assert set(owner[_np(got[2]["face_map"])]) == {0} and got[1].shape[0] == 500
    rest = f[owner != 0]                                                     # without the sheet the two 20-face pieces tie
    got = _clean(v, rest, keep_largest=True)
    want = ref.clean(v, rest, keep_largest=True)
    _same_clean(got, want)
    labels = want["labels"]
    tie = sorted({int(labels[x]) for x in rest[np.isin(owner[owner != 0], (5, 6))][:, 0]})
    assert len(tie) == 2 and got[1].shape[0] == 20
    assert set(labels[rest[_np(got[2]["face_map"])][:, 0]]) == {tie[0]}      # the lower label wins


def test_clean_mesh_edge_cases():
    from gaussianip_amd import _lib
    v, f, _ = inputs.clean_scene()
    before = dict(_lib.call_counts)
    gv, gf, info = _clean(v, np.zeros((0, 3), np.int32))
    assert dict(_lib.call_counts) == before                                  # F == 0: no launch
    assert gv.shape == (0, 3) and gf.shape == (0, 3) and info["face_map"].shape == (0,) and info["num_components"] == 0
    assert np.array_equal(_np(info["vertex_map"]), np.full(len(v), -1)) and np.array_equal(_np(info["labels"]), np.arange(len(v)))
    bad = f.copy()
    bad[3, 1], bad[40, 0] = len(v), -2
    with pytest.raises(ValueError):
        _clean(v, bad)
    _same_clean(_clean(v, bad, validate=False), ref.clean(v, bad))           # skipped by the kernels, dropped from the output


# ---------------------------------------------------------------------------------------------------------------- 3. cluster_decimate
@functools.lru_cache(maxsize=None)
def _surface():
    """The iso-surface of tests/field_inputs.py case a at R = 32 (vertices in grid-index units), extracted once."""
    from gaussianip_amd.utils.mesh import extract_surface
    cl, R, nb = field_inputs.case("a")
    occ = _model(cl).extract_fields(R, nb)
    thr = float(torch.quantile(occ.reshape(-1), 0.8))
    v, f = extract_surface(occ, thr)
    assert f.shape[0] > 5000, f.shape
    return v, f, _np(v), _np(f)


@functools.lru_cache(maxsize=None)
def _surface_reference(n):
    _, _, v, f = _surface()
    return ref.cluster(v, f, n, np.float64), ref.cluster(v, f, n, np.float32)


def _bar(name, got, f64, f32):
    got, f64, f32 = (np.asarray(a, np.float64) for a in (got, f64, f32))
    ref_err = float(np.abs(f32 - f64).max())
    err = float(np.abs(got - f64).max())
    bar = FACTOR * ref_err
    print("%s: kernel %.3e, float32 restatement %.3e, bar %.3e" % (name, err, ref_err, bar))
    _figures[name] = dict(kernel_err=err, restatement_err=ref_err, bar=bar)
    assert np.isfinite(got).all() and ref_err > 0 and err <= bar, (name, err, ref_err, bar)
    return bar


@pytest.mark.parametrize("n", [5, 12])
def test_cluster_decimate_against_the_restatement(n):
    from gaussianip_amd.utils.mesh import cluster_decimate
    tv, tf, v, f = _surface()
    want64, want32 = _surface_reference(n)
    for lanes in (None, 16, 32, 64):
        gv, gf, vm = cluster_decimate(tv, tf, n, lanes=lanes)
        assert gv.dtype == torch.float32 and gf.dtype == torch.int32 and vm.dtype == torch.int32 and vm.shape == (len(v),)
        assert np.array_equal(_np(gf), want64["faces"]) and np.array_equal(_np(vm), want64["vertex_map"])
        name = "surface_R32_grid%d" % n if lanes is None else "surface_R32_grid%d_lanes%d" % (n, lanes)
        _bar(name, _np(gv), want64["vertices"], want32["vertices"])
    _figures["surface_R32_grid%d" % n].update(faces_in=int(len(f)), faces_out=int(gf.shape[0]), vertices_out=int(gv.shape[0]),
                                              cell=float(want64["h"]))


def test_cluster_decimate_validity_containment_and_reproducibility():
    from gaussianip_amd.utils.mesh import cluster_decimate
    tv, tf, v, f = _surface()
    for n in (5, 12, 40):
        gv, gf, vm = cluster_decimate(tv, tf, n)
        again = cluster_decimate(tv, tf, n)
        assert torch.equal(gv, again[0]) and torch.equal(gf, again[1]) and torch.equal(vm, again[2])      # bit for bit
        out, faces, vmap = _np(gv), _np(gf).astype(np.int64), _np(vm)
        h = float(ref.grid_frame(v, n)[1])
        inside = vmap >= 0
        assert inside.any() and vmap.max() == len(out) - 1
        dist = np.linalg.norm(v[inside].astype(np.float64) - out[vmap[inside]], axis=1)
        assert dist.max() <= math.sqrt(3) * h * (1 + 1e-5)                                                 # the clamp
        assert not ((faces[:, 0] == faces[:, 1]) | (faces[:, 1] == faces[:, 2]) | (faces[:, 0] == faces[:, 2])).any()
        assert len(np.unique(np.sort(faces, 1), axis=0)) == len(faces)                                     # no corner set twice
        assert np.array_equal(np.unique(faces), np.arange(len(out)))                                       # every vertex is referenced
        assert len(faces) <= ref.face_count(v, f, n) < len(f)


def test_cluster_decimate_boundary_vertices():
    from gaussianip_amd.utils.mesh import cluster_decimate, cluster_face_count
    v, f = inputs.dyadic_boundary()
    want = ref.cluster(v, f, 8)
    assert np.array_equal(ref.cell_indices(v, 8)[0], ref.cell_indices_exact(v, 8)[0])
    gv, gf, vm = cluster_decimate(_cu(v), _cu(f), 8)
    assert np.array_equal(_np(vm), want["vertex_map"]) and np.array_equal(_np(gf), want["faces"])
    assert cluster_face_count(_cu(v), _cu(f), 8) == ref.face_count(v, f, 8)
    assert np.abs(_np(gv) - want["vertices"]).max() <= 0.125 * math.sqrt(3)      # positions: only that they are the same cells' (the clamp)


def test_cluster_decimate_flat_patch():
    from gaussianip_amd.utils.mesh import cluster_decimate
    v, f, normal, origin = inputs.flat_patch()
    want64, want32 = ref.cluster(v, f, 6, np.float64), ref.cluster(v, f, 6, np.float32)
    gv, gf, vm = cluster_decimate(_cu(v), _cu(f), 6)
    assert np.array_equal(_np(gf), want64["faces"]) and np.array_equal(_np(vm), want64["vertex_map"])
    bar = _bar("flat_patch_grid6", _np(gv), want64["vertices"], want32["vertices"])
    out = _np(gv).astype(np.float64)
    off_plane = np.abs((out - origin) @ normal).max()
    off_mean = np.abs(out - want64["mean"][want64["new_id"] >= 0]).max()
    print("flat patch: %d vertices, off the plane %.3e, off the members' mean %.3e, bar %.3e" % (len(out), off_plane, off_mean, bar))
    _figures["flat_patch_grid6"].update(off_plane=float(off_plane), off_mean=float(off_mean))
    assert len(out) >= 20 and off_plane <= bar and off_mean <= bar


def test_cluster_decimate_cube_corners():
    from gaussianip_amd.utils.mesh import cluster_decimate
    v, f = inputs.cube()
    n = inputs.CUBE_GRID
    want = ref.cluster(v, f, n)
    gv, gf, vm = cluster_decimate(_cu(v), _cu(f), n)
    assert np.array_equal(_np(gf), want["faces"]) and np.array_equal(_np(vm), want["vertex_map"])
    assert (_np(vm)[-2:] == -1).all()                                     # the two vertices that only widen the grid are gone
    h = float(want["h"])
    bound = 3 * ref.LAMBDA / (1 + 3 * ref.LAMBDA) * math.sqrt(3) * h
    out, worst, worst_mean = _np(gv).astype(np.float64), 0.0, np.inf
    for corner in [(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)]:
        c = np.nonzero((want["cells"] == [1 if s < 0 else n - 2 for s in corner]).all(1))[0]
        assert len(c) == 1
        lo_edge = want["lo"].astype(np.float64) + want["cells"][c[0]] * h
        assert ((np.array(corner) > lo_edge + 0.25 * h) & (np.array(corner) < lo_edge + 0.75 * h)).all()      # strictly inside its cell
        worst = max(worst, float(np.linalg.norm(out[want["new_id"][c[0]]] - np.array(corner, np.float64))))
        worst_mean = min(worst_mean, float(np.linalg.norm(want["mean"][c[0]] - np.array(corner, np.float64))))
    print("cube corners: worst distance %.3e, bound %.3e; the members' mean is at least %.3e away" % (worst, bound, worst_mean))
    _figures["cube_corners"] = dict(worst=worst, bound=bound, mean_distance=worst_mean, cell=h)
    assert worst <= bound
    assert worst_mean > bound                                             # the mean does not meet it: the quadric does the work


def test_cluster_decimate_size_extremes():
    from gaussianip_amd.utils.mesh import cluster_decimate
    tv, tf, v, f = _surface()
    gv, gf, vm = cluster_decimate(tv, tf, 1)
    assert gf.shape == (0, 3) and gv.shape == (0, 3) and (vm == -1).all()
    cv, cf = inputs.unit_cube()
    gv, gf, vm = cluster_decimate(_cu(cv), _cu(cf), 2048)
    assert np.array_equal(_np(gf), cf) and np.array_equal(_np(vm), np.arange(8))
    assert np.abs(_np(gv) - cv).max() <= 1.0 / 2048                       # each vertex alone in its cell: it stays inside it
    with pytest.raises(ValueError):
        cluster_decimate(torch.zeros((5, 3), device="cuda"), _cu(cf[:1] * 0), 4)      # no extent
    for grid in (0, 2049, 2.5):
        with pytest.raises(ValueError):
            cluster_decimate(_cu(cv), _cu(cf), grid)
    with pytest.raises(ValueError):
        cluster_decimate(_cu(cv), _cu(cf), 4, lanes=8)


# ---------------------------------------------------------------------------------------------------------------- 4. decimate_mesh
@pytest.mark.parametrize("target", [50, 500, 5000])
def test_decimate_mesh_meets_its_target(target):
    from gaussianip_amd import _lib
    from gaussianip_amd.utils.mesh import cluster_decimate, cluster_face_count, decimate_mesh
    tv, tf, v, f = _surface()
    before = _lib.call_counts.get("gip_mesh_cluster_count", 0)
    gv, gf, vm, grid = decimate_mesh(tv, tf, target)
    probes = _lib.call_counts.get("gip_mesh_cluster_count", 0) - before
    assert 1 <= grid < 2048 and probes <= 12
    assert gf.shape[0] <= target
    lo, hi = cluster_face_count(tv, tf, grid), cluster_face_count(tv, tf, grid + 1)
    print("target %d: grid %d, %d faces (count %d, next grid's %d), %d probes" % (target, grid, gf.shape[0], lo, hi, probes))
    _figures["decimate_target%d" % target] = dict(grid=grid, faces=int(gf.shape[0]), count=lo, next_count=hi, probes=probes)
    assert lo <= target < hi
    assert lo == ref.face_count(v, f, grid) and hi == ref.face_count(v, f, grid + 1)
    want = cluster_decimate(tv, tf, grid)
    assert torch.equal(gv, want[0]) and torch.equal(gf, want[1]) and torch.equal(vm, want[2])


def test_decimate_mesh_large_targets_and_errors():
    from gaussianip_amd.utils.mesh import decimate_mesh
    tv, tf, v, f = _surface()
    for target in (len(f), len(f) + 1, 10 ** 9):
        gv, gf, vm, grid = decimate_mesh(tv, tf, target)
        assert grid == 0 and gv is tv and gf is tf and np.array_equal(_np(vm), np.arange(len(v)))
    for target in (0, -3, 0.5):
        with pytest.raises(ValueError):
            decimate_mesh(tv, tf, target)
    cv, cf = inputs.unit_cube()
    more = np.concatenate((cf[:5], [[0, 0, 1], [2, 3, 3], [7, 7, 7]], cf[5:])).astype(np.int32)      # 15 faces, three of them collapsed
    gv, gf, vm, grid = decimate_mesh(_cu(cv), _cu(more), 12)                # count(2048) == 12 fits the target: the grid is 2048
    assert grid == 2048 and np.array_equal(_np(gf), cf) and np.array_equal(_np(vm), np.arange(8))
    gv, gf, vm, grid = decimate_mesh(_cu(cv), _cu(more), 11)                # every grid above 1 keeps all 12: only the single cell fits
    assert grid == 1 and gf.shape[0] == 0


# ---------------------------------------------------------------------------------------------------------------- 5. end to end
R, NB, THR = 64, 8, 1.0
FLOATER = np.array([0.8, 0.8, 0.8], np.float32)


@functools.lru_cache(maxsize=None)
def _blob():
    """The blob cloud of the mesh tests and, away from it, three coincident Gaussians (sigma 0.02, opacity 0.8 each: a peak density of
    2.4, a sphere of radius sigma sqrt(2 ln 2.4) = 0.026 at density 1, a box diagonal of 0.09): a floater of 4 % of the scene's diagonal
    (the box from -0.5 to 0.83 per axis: 2.3), and about one grid spacing in radius."""
    cl = dict(sample_inputs.blob_cloud())
    P = cl["xyz"].shape[0]
    rot = np.zeros((3, 4), np.float32)
    rot[:, 0] = 1
    cl["xyz"] = np.concatenate((cl["xyz"], np.tile(FLOATER, (3, 1)))).astype(np.float32)
    cl["opacity"] = np.concatenate((cl["opacity"], np.full((3, 1), math.log(0.8 / 0.2), np.float32))).astype(np.float32)
    cl["scaling"] = np.concatenate((cl["scaling"], np.full((3, 3), math.log(0.02), np.float32))).astype(np.float32)
    cl["rotation"] = np.concatenate((cl["rotation"], rot)).astype(np.float32)
    rgb = sample_inputs.colors(P + 3, 9)
    gm = _model(cl, rgb)
    return gm, gm.extract_textured_mesh(density_thresh=THR, resolution=R, num_blocks=NB)


def test_defaults_change_nothing():
    gm, plain = _blob()
    explicit = gm.extract_textured_mesh(density_thresh=THR, resolution=R, num_blocks=NB, clean=False, min_faces=8, min_diameter=0.05,
                                        decimate_target=0)
    assert all(torch.equal(a, b) for a, b in zip(plain, explicit))
    v, f = gm.extract_mesh(density_thresh=THR, resolution=R, num_blocks=NB, clean=False, decimate_target=0)
    assert torch.equal(v, plain[0]) and torch.equal(f, plain[1])


def test_clean_alone_selects_rows():
    from gaussianip_amd.utils.mesh import clean_mesh
    gm, (v0, f0, n0, _, _) = _blob()
    kw = dict(density_thresh=THR, resolution=R, num_blocks=NB)
    _, _, _, c0 = gm.extract_mesh_with_attributes(**kw)
    v, f, n, c = gm.extract_mesh_with_attributes(clean=True, **kw)
    cv, cf, info = clean_mesh(v0, f0)
    rows = torch.nonzero(info["vertex_map"] >= 0).reshape(-1)
    print("blob with a floater: %d -> %d faces, %d of %d components kept" % (f0.shape[0], f.shape[0], info["num_kept"], info["num_components"]))
    assert info["num_kept"] < info["num_components"] and 0 < f.shape[0] < f0.shape[0]          # the floater is there, and goes
    assert float((v - _cu(FLOATER)).norm(dim=1).min()) > 0.3 and float((v0 - _cu(FLOATER)).norm(dim=1).min()) < 0.1
    assert torch.equal(v, v0[rows]) and torch.equal(v, cv) and torch.equal(f, cf)
    assert torch.equal(n, n0[rows]) and torch.equal(c, c0[rows])
    assert torch.equal(f0[info["face_map"].long()].long(), rows[f.long()])
    tv, tf, tn, _, _ = gm.extract_textured_mesh(clean=True, **kw)
    assert torch.equal(tv, v) and torch.equal(tf, f) and torch.equal(tn, n)
    mv, mf = gm.extract_mesh(clean=True, **kw)
    assert torch.equal(mv, v) and torch.equal(mf, f)


def _camera(el, az, dist, target, fovy_deg, size):
    from gaussianip_amd.scene import Camera
    c2w = scenes.orbit_c2w(el, az, dist)
    rot = c2w[:3, :3].clone()
    c2w[:3, 3] -= rot @ torch.diag(torch.tensor([1.0, -1.0, -1.0])) @ rot.t() @ torch.tensor(target, dtype=torch.float32)
    return Camera(c2w=c2w.cuda(), FoVy=math.radians(fovy_deg), height=size, width=size)


def test_clean_and_decimate_end_to_end(tmp_path):
    from gaussianip_amd.utils.mesh import read_obj_textured
    from gaussianip_amd.utils.rasterize import render_mesh
    gm, (v0, f0, _, _, tex0) = _blob()
    kw = dict(density_thresh=THR, resolution=R, num_blocks=NB, clean=True, decimate_target=2000)
    obj = tmp_path / "out" / "small.obj"
    v, f, n, uv, texture = gm.extract_textured_mesh(path=str(obj), texture_size=int(tex0.shape[0]), **kw)
    assert 0 < f.shape[0] <= 2000 < f0.shape[0] and v.shape[0] < v0.shape[0] and n.shape == v.shape and uv.shape == (f.shape[0], 3, 2)
    assert int(f.min()) == 0 and int(f.max()) == v.shape[0] - 1
    norms = n.norm(dim=1)
    assert float((norms - 1).abs().max()) < 1e-5                                         # sampled at the new vertices
    cell0 = gm.bake_texture(v0, f0, int(tex0.shape[0]), resolution=R, num_blocks=NB)["cell"]
    cell = gm.bake_texture(v, f, int(tex0.shape[0]), resolution=R, num_blocks=NB)["cell"]
    print("%d -> %d faces; atlas cell at T = %d: %d -> %d" % (f0.shape[0], f.shape[0], tex0.shape[0], cell0, cell))
    _figures["end_to_end"] = dict(faces_in=int(f0.shape[0]), faces_out=int(f.shape[0]), texture=int(tex0.shape[0]), cell_in=cell0, cell_out=cell)
    assert cell >= cell0
    rv, rf, rn, ruv, rtex = read_obj_textured(str(obj))
    assert np.array_equal(rv, _np(v)) and np.array_equal(rf, _np(f)) and np.array_equal(rn, _np(n)) and np.array_equal(ruv, _np(uv))
    assert rtex.shape == tuple(texture.shape) and np.abs(rtex - _np(texture)).max() <= 0.5 / 255 + 1e-7
    cam = _camera(20.0, 35.0, 2.2, (0.0, 0.0, 0.0), 50.0, 128)
    out = gm.render_textured_mesh(cam, position_gradients=True, antialias=True, texture_size=int(tex0.shape[0]), **kw)
    assert torch.equal(out["mesh"][0], v) and torch.equal(out["mesh"][1], f) and float(out["alpha"].sum()) > 500
    verts = v.clone().requires_grad_(True)
    alpha = render_mesh(cam, verts, f, uv, texture, position_gradients=True, antialias=True)["alpha"]
    (alpha ** 2).sum().backward()
    assert verts.grad is not None and bool(torch.isfinite(verts.grad).all()) and bool(verts.grad.any())
