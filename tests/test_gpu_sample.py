"""The field sampler on the GPU (csrc/field_sample.hip, GaussianModel.sample_fields / extract_mesh_with_attributes).

Float64 side: tests/sample_reference.py.  Bar, errors normalised by the output's maximum: at most 4 times the float32 error of the
comparison's own reference against float64 plus a floor of 2e-6 — the rule of tests/test_gpu_field.py.  For the grid-point test the
reference is the stored float32 field of tests/golden/field.npz and `err` is the fixture's; for the off-grid test it is
sample_reference in float32 against itself in float64 on the same inputs, computed here and printed."""
import functools

import numpy as np
import pytest
import torch

import field_inputs
import sample_inputs
import sample_reference

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 4.0, 2e-6


def _model(cl, colors=None):
    from gaussianip_amd.scene import GaussianModel
    from gaussianip_amd.utils.sh import C0
    gm = GaussianModel(0)
    gm._xyz, gm._opacity = torch.from_numpy(cl["xyz"]).cuda(), torch.from_numpy(cl["opacity"]).cuda()
    gm._scaling, gm._rotation = torch.from_numpy(cl["scaling"]).cuda(), torch.from_numpy(cl["rotation"]).cuda()
    P = cl["xyz"].shape[0]
    rgb = np.full((P, 3), 0.5, np.float32) if colors is None else colors
    gm._features_dc = ((torch.from_numpy(rgb).cuda() - 0.5) / C0).reshape(P, 1, 3).contiguous()
    return gm


def _sample(gm, *args, **kw):
    from gaussianip_amd import _lib
    before = _lib.call_counts.get("gip_field_sample", 0)
    out = gm.sample_fields(*args, **kw)
    assert set(out) == {"density", "gradient", "color"}
    V = args[0].shape[0]
    assert out["density"].shape == (V,) and out["gradient"].shape == (V, 3) and out["color"].shape == (V, 3)
    assert all(t.dtype == torch.float32 and t.is_cuda for t in out.values())
    if V and int((torch.sigmoid(gm._opacity) > 0.005).sum()):
        assert _lib.call_counts.get("gip_field_sample", 0) == before + 1      # the HIP path ran
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. grid points
@pytest.mark.parametrize("name", ["a", "b"])
def test_grid_points_match_the_reference_field(name):
    golden = field_inputs.load_golden()
    cl, R, nb = field_inputs.case(name)
    want = golden[name + "_field"].astype(np.float64).reshape(-1)
    gm = _model(cl)
    out = _sample(gm, sample_inputs.grid_points(R).cuda(), resolution=R, num_blocks=nb, normalized=True)
    got = out["density"]
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max() / np.abs(want).max())
    bar = FACTOR * float(golden[name + "_err"]) + FLOOR
    print("case %s: sampler vs the reference's float32 field %.3e, bar %.3e" % (name, err, bar))
    assert torch.isfinite(got).all() and torch.isfinite(out["gradient"]).all() and torch.isfinite(out["color"]).all()
    assert err <= bar
    # the same batching and the same fmaf chain as field.hip: bit for bit the voxels of extract_fields
    occ = gm.extract_fields(resolution=R, num_blocks=nb)
    assert torch.equal(got, occ.reshape(-1))


@pytest.mark.parametrize("R,nb", [(17, 1), (34, 2)])
def test_grid_points_equal_the_field_on_its_second_pass(R, nb):
    """Blocks of 4913 voxels: the field kernel holds 16 voxels per lane and makes two passes, the sampler five of four points."""
    cl, R, nb = field_inputs.large_block_case(R, nb)
    gm = _model(cl)
    out = _sample(gm, sample_inputs.grid_points(R).cuda(), resolution=R, num_blocks=nb, normalized=True)
    occ = gm.extract_fields(resolution=R, num_blocks=nb)
    assert float(occ.max()) > 0 and torch.equal(out["density"], occ.reshape(-1))


# ---------------------------------------------------------------------------------------------------------------- 2. off-grid points
@functools.lru_cache(maxsize=None)
def _offgrid():
    cl, R, nb = field_inputs.case("b")
    rgb = sample_inputs.colors(cl["xyz"].shape[0], 5)
    u, blk = sample_inputs.offgrid_points(R, nb)
    args = (cl["xyz"], cl["opacity"], cl["scaling"], cl["rotation"], rgb, R, nb, u, blk)
    f64 = sample_reference.sample_sums(*args, dtype=np.float64)
    f32 = sample_reference.sample_sums(*args, dtype=np.float32)
    return cl, R, nb, rgb, u, blk, f64, f32


def test_offgrid_points_against_float64():
    cl, R, nb, rgb, u, blk, f64, f32 = _offgrid()
    info = f64[3]
    assert info["face_distance"] > 1e-5                       # float32 and float64 agree about every member
    assert np.array_equal(info["keep"], f32[3]["keep"]) and np.array_equal(info["members"], f32[3]["members"])
    counts = np.bincount(blk, minlength=nb ** 3)
    assert counts.max() > sample_inputs.ONE_PASS and (counts == 0).any() and (counts == 1).any()
    assert info["members"].max() > 2048                       # the member list is flushed in mid-walk
    assert (np.abs(u) > 1).any()                              # points outside the grid
    gm = _model(cl, rgb)
    pts = torch.from_numpy(u).cuda()
    out = _sample(gm, pts, colors=torch.from_numpy(rgb).cuda(), resolution=R, num_blocks=nb, normalized=True)
    dens = out["density"].cpu().numpy().astype(np.float64)
    # the raw sums from the public outputs, in float64: gradient back to normalised units, color * density = color_sum up to the
    # one float32 rounding of the division (6e-8 of the value, far below the floor)
    got = {"density": dens, "gradient": out["gradient"].cpu().numpy().astype(np.float64) / gm.scale,
           "color_sum": out["color"].cpu().numpy().astype(np.float64) * dens[:, None]}
    for i, key in enumerate(("density", "gradient", "color_sum")):
        mx = np.abs(f64[i]).max()
        ref_err = float(np.abs(f32[i].astype(np.float64) - f64[i]).max() / mx)
        err = float(np.abs(got[key] - f64[i]).max() / mx)
        bar = FACTOR * ref_err + FLOOR
        print("%s: kernel %.3e reference %.3e bar %.3e" % (key, err, ref_err, bar))
        assert np.isfinite(got[key]).all()
        assert err <= bar, (key, err, ref_err)
    # the default colour is the base colour of features_dc, which _model set from the same rgb
    base = _sample(gm, pts, resolution=R, num_blocks=nb, normalized=True)
    assert torch.equal(base["density"], out["density"]) and float((base["color"] - out["color"]).abs().max()) <= 1e-5
    # outputs follow the caller's order
    perm = torch.from_numpy(np.random.default_rng(3).permutation(len(u))).cuda()
    shuffled = _sample(gm, pts[perm].contiguous(), colors=torch.from_numpy(rgb).cuda(), resolution=R, num_blocks=nb, normalized=True)
    for key in ("density", "gradient", "color"):
        assert torch.equal(shuffled[key], out[key][perm]), key


def test_world_coordinates_are_normalised_like_the_field():
    cl, R, nb, rgb, u, _, _, _ = _offgrid()
    gm = _model(cl, rgb)
    direct = _sample(gm, torch.from_numpy(u[:500]).cuda(), resolution=R, num_blocks=nb, normalized=True)
    world = torch.from_numpy(u[:500]).cuda() / gm.scale + gm.center
    back = (world - gm.center) * gm.scale                     # what sample_fields makes of world points, with float32 rounding
    via = _sample(gm, world, resolution=R, num_blocks=nb)
    again = _sample(gm, back.contiguous(), resolution=R, num_blocks=nb, normalized=True)
    assert torch.equal(via["density"], again["density"]) and torch.equal(via["gradient"], again["gradient"])
    assert float((via["density"] - direct["density"]).abs().max()) <= 1e-3 * float(direct["density"].max())


# ---------------------------------------------------------------------------------------------------------------- 3, 4. one Gaussian
@functools.lru_cache(maxsize=None)
def _sphere():
    cl, rgb = sample_inputs.sphere_cloud()
    gm = _model(cl, rgb)
    v, f, n, c = gm.extract_mesh_with_attributes(density_thresh=sample_inputs.SPHERE_THRESHOLD, resolution=32, num_blocks=4)
    v0, f0 = _model(cl, rgb).extract_mesh(density_thresh=sample_inputs.SPHERE_THRESHOLD, resolution=32, num_blocks=4)
    return gm, v, f, n, c, v0, f0


def test_one_isotropic_gaussian():
    gm, v, f, n, c, _, _ = _sphere()
    assert v.shape[0] > 100 and n.shape == v.shape and c.shape == v.shape and n.dtype == c.dtype == torch.float32
    vd = v.cpu().numpy().astype(np.float64)
    d = vd - sample_inputs.SPHERE_MU.astype(np.float32).astype(np.float64)
    r = np.linalg.norm(d, axis=1)
    spacing = 2 / 31 / gm.scale                               # one grid spacing in world units
    assert abs(gm.scale - 1.8) <= 1e-6
    print("radius: analytic %.5f, vertices %.5f .. %.5f, grid spacing %.5f" % (sample_inputs.SPHERE_RADIUS, r.min(), r.max(), spacing))
    assert np.abs(r - sample_inputs.SPHERE_RADIUS).max() <= spacing
    nerr = np.abs(n.cpu().numpy().astype(np.float64) - d / r[:, None]).max()
    # the two far Gaussians' weight at the vertices, in float64: below float32 resolution of the density there
    far = sum(sample_inputs.FAR_OPACITY * np.exp(-((vd - p) ** 2).sum(1) / (2 * sample_inputs.FAR_SIGMA ** 2)) for p in sample_inputs.FAR_XYZ)
    assert far.max() <= 2.0 ** -25 * sample_inputs.SPHERE_THRESHOLD
    cerr = np.abs(c.cpu().numpy().astype(np.float64) - np.array(sample_inputs.SPHERE_COLOR, np.float32).astype(np.float64)).max()
    print("normal error %.3e, colour error %.3e" % (nerr, cerr))
    assert nerr <= 1e-4
    assert cerr <= 1e-5


def test_normals_agree_with_the_winding():
    _, v, f, n, _, v0, f0 = _sphere()
    assert torch.equal(v, v0) and torch.equal(f, f0)          # extract_mesh's tensors, bit for bit
    vd, fl = v.double(), f.long()
    fn = torch.cross(vd[fl[:, 1]] - vd[fl[:, 0]], vd[fl[:, 2]] - vd[fl[:, 0]], dim=1)       # length = twice the face's area
    acc = torch.zeros_like(vd)
    for k in range(3):
        acc.index_add_(0, fl[:, k], fn)
    has_area = acc.norm(dim=1) > 0
    assert int(has_area.sum()) > 100
    assert ((acc * n.double()).sum(1)[has_area] > 0).all()


# ---------------------------------------------------------------------------------------------------------------- 5. edges
def test_no_points():
    cl, R, nb = field_inputs.edge_case("repeat")
    out = _sample(_model(cl), torch.zeros((0, 3), device="cuda"), resolution=R, num_blocks=nb)
    assert out["density"].numel() == 0 and out["gradient"].numel() == 0 and out["color"].numel() == 0


def test_nothing_passes_the_prefilter():
    cl, R, nb = field_inputs.edge_case("transparent")
    pts = torch.from_numpy(np.random.default_rng(1).uniform(-0.5, 0.5, (300, 3)).astype(np.float32)).cuda()
    for normalized in (False, True):
        out = _sample(_model(cl), pts, resolution=R, num_blocks=nb, normalized=normalized)
        for t in out.values():
            assert torch.equal(t, torch.zeros_like(t))        # colour 0, not NaN


def test_points_outside_the_grid_and_repeatability():
    cl, R, nb = field_inputs.edge_case("repeat")
    rng = np.random.default_rng(2)
    u = rng.uniform(-1.5, 1.5, (2000, 3)).astype(np.float32)
    u[:6] = [[-3, 0, 0], [3, 0, 0], [0, -3, 0], [0, 3, 0], [0.1, 0.1, -1.0001], [1.0001, 1.0001, 1.0001]]
    pts = torch.from_numpy(u).cuda()
    first = _sample(_model(cl), pts, resolution=R, num_blocks=nb, normalized=True)
    second = _sample(_model(cl), pts, resolution=R, num_blocks=nb, normalized=True)
    assert float(first["density"].max()) > 0
    for key in first:
        assert torch.isfinite(first[key]).all() and torch.equal(first[key], second[key]), key


def test_argument_errors():
    cl, R, nb = field_inputs.edge_case("single")
    gm = _model(cl)
    pts = torch.zeros((4, 3), device="cuda")
    with pytest.raises(ValueError):
        gm.sample_fields(torch.zeros(4, 3), resolution=R, num_blocks=nb)              # not on the GPU
    with pytest.raises(ValueError):
        gm.sample_fields(torch.zeros((4, 2), device="cuda"), resolution=R, num_blocks=nb)
    with pytest.raises(ValueError):
        gm.sample_fields(torch.zeros(12, device="cuda"), resolution=R, num_blocks=nb)
    with pytest.raises(ValueError, match="divide"):
        gm.sample_fields(pts, resolution=30, num_blocks=16)
    with pytest.raises(ValueError, match="divide"):
        gm.extract_mesh_with_attributes(resolution=30, num_blocks=16)
    with pytest.raises(ValueError):
        gm.sample_fields(pts, colors=torch.zeros((5, 3), device="cuda"), resolution=R, num_blocks=nb)


# ---------------------------------------------------------------------------------------------------------------- 6. end to end
def test_mesh_with_attributes_end_to_end(tmp_path):
    from gaussianip_amd.utils.mesh import read_obj_full, read_ply_mesh
    cl = sample_inputs.blob_cloud()
    rgb = sample_inputs.colors(cl["xyz"].shape[0], 9)
    R, nb, thr = 64, 8, 1.0
    gm = _model(cl, rgb)
    ply, obj = tmp_path / "out" / "mesh.ply", tmp_path / "out" / "mesh.obj"
    v, f, n, c = gm.extract_mesh_with_attributes(path=str(ply), density_thresh=thr, resolution=R, num_blocks=nb)
    v2, f2, n2, c2 = gm.extract_mesh_with_attributes(path=str(obj), density_thresh=thr, resolution=R, num_blocks=nb)
    for x, y in ((v, v2), (f, f2), (n, n2), (c, c2)):
        assert torch.equal(x, y)
    v0, f0 = gm.extract_mesh(density_thresh=thr, resolution=R, num_blocks=nb)
    assert torch.equal(v, v0) and torch.equal(f, f0) and v.shape[0] > 1000
    vn, fn, nn, cn = (t.cpu().numpy() for t in (v, f, n, c))
    pv, pf, pc, pn = read_ply_mesh(str(ply))
    assert np.array_equal(pv, vn) and np.array_equal(pf, fn) and np.array_equal(pn, nn)
    assert np.abs(pc - cn).max() <= 1 / 255
    ov, of, oc, on = read_obj_full(str(obj))
    assert np.array_equal(ov, vn) and np.array_equal(of, fn) and np.array_equal(on, nn) and np.array_equal(oc, cn)
    length = n.double().norm(dim=1)
    assert (((length - 1).abs() <= 1e-5) | ((n == 0).all(1))).all()
    assert float(c.min()) >= 0 and float(c.max()) <= 1
    # density at the vertices: a vertex lies on a crossing edge, between a grid value below the threshold and one at or above it;
    # the bound is the largest step between the two ends of any crossing edge of this field
    occ = gm.extract_fields(resolution=R, num_blocks=nb)
    bound = 0.0
    for d in range(1, 8):
        di, dj, dk = d & 1, (d >> 1) & 1, (d >> 2) & 1
        f0_ = occ[:R - di, :R - dj, :R - dk]
        f1_ = occ[di:, dj:, dk:]
        cross = (f0_ >= thr) != (f1_ >= thr)
        if bool(cross.any()):
            bound = max(bound, float((f1_ - f0_).abs()[cross].max()))
    dens = gm.sample_fields(v, resolution=R, num_blocks=nb)["density"]
    dev = float((dens - thr).abs().max())
    print("%d vertices: |density - threshold| at most %.4f, bound %.4f" % (v.shape[0], dev, bound))
    assert 0 < bound and dev <= bound
