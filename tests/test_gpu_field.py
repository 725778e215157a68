"""The density field on the GPU (csrc/field.hip, GaussianModel.extract_fields).

Float64 side: tests/field_reference.py (checked against the reference's own float64 numbers in tests/test_field_cpu.py); for case c
the 4096 float64 samples of tests/golden/field.npz.  Bar, errors normalised by the field's maximum: the kernel's error against float64
is at most 4 times the REFERENCE's own float32 error against float64 (`err` of tests/golden/field.npz, tools/make_golden.py group
`field`) plus a floor of 2e-6 — the form and the factor of tests/test_gpu_ssim.py.  The edge cases have no run of the reference; they
take the smallest `err` of the three stored cases.  Every comparison first checks that no centre lies within 1e-5 of a box face it
is tested against (float32 and float64 then agree about every member; float32 rounding of a normalised centre is ~1e-7).

With GIP_FIELD_PARITY_OUT=<file> the per-case figures are written there as JSON (profiles/field_parity.json is such a run)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import field_inputs
import field_reference

pytestmark = pytest.mark.gpu
FACTOR, FLOOR = 4.0, 2e-6
_figures = {}


@pytest.fixture(scope="module")
def golden():
    yield field_inputs.load_golden()
    out = os.environ.get("GIP_FIELD_PARITY_OUT")
    if out and _figures:
        with open(out, "w") as f:
            json.dump(_figures, f, indent=1, sort_keys=True)


def _model(cl):
    from gaussianip_amd.scene import GaussianModel
    gm = GaussianModel(0)
    gm._xyz, gm._opacity = torch.from_numpy(cl["xyz"]).cuda(), torch.from_numpy(cl["opacity"]).cuda()
    gm._scaling, gm._rotation = torch.from_numpy(cl["scaling"]).cuda(), torch.from_numpy(cl["rotation"]).cuda()
    return gm


def _kernel(cl, R, nb):
    from gaussianip_amd import _lib
    before = _lib.call_counts.get("gip_density_field", 0)
    gm = _model(cl)
    occ = gm.extract_fields(resolution=R, num_blocks=nb)
    assert occ.shape == (R, R, R) and occ.dtype == torch.float32 and occ.is_cuda
    if int((torch.sigmoid(gm._opacity) > 0.005).sum()):
        assert _lib.call_counts.get("gip_density_field", 0) == before + 1
    return occ, gm


@functools.lru_cache(maxsize=None)
def _edge_reference(name):
    cl, R, nb = field_inputs.edge_case(name)
    return field_reference.density_field(cl["xyz"], cl["opacity"], cl["scaling"], cl["rotation"], R, nb)


def _check(key, got, want, mx, ref_err):
    err = float(np.abs(got.astype(np.float64) - want).max() / mx)
    bar = FACTOR * ref_err + FLOOR
    _figures[key] = {"kernel_err": err, "reference_err": ref_err, "ratio": err / ref_err, "bar": bar}
    print("%s: kernel %.3e reference %.3e bar %.3e" % (key, err, ref_err, bar))
    assert np.isfinite(got).all()
    assert err <= bar, (key, err, ref_err)


@pytest.mark.parametrize("name", ["a", "b"])
def test_full_field_against_float64(golden, name):
    cl, R, nb = field_inputs.case(name)
    f64, info = field_reference.density_field(cl["xyz"], cl["opacity"], cl["scaling"], cl["rotation"], R, nb)
    assert info["face_distance"] > 1e-5
    occ, gm = _kernel(cl, R, nb)
    _check("case_" + name, occ.cpu().numpy(), f64, np.abs(f64).max(), float(golden[name + "_err"]))
    np.testing.assert_allclose(gm.center.cpu().numpy(), golden[name + "_center"], rtol=0, atol=1e-7)
    assert abs(gm.scale - float(golden[name + "_scale"])) <= 2e-7 * gm.scale
    empty = torch.from_numpy(np.repeat(np.repeat(np.repeat(info["members"] == 0, R // nb, 0), R // nb, 1), R // nb, 2)).cuda()
    assert (occ[empty] == 0).all()              # (these clouds may leave no block empty; the octant case always does)


def test_default_geometry_samples_against_float64(golden):
    cl, R, nb = field_inputs.case("c")
    occ, gm = _kernel(cl, R, nb)
    at = torch.from_numpy(field_inputs.sample_voxels(R)).cuda()
    _check("case_c", occ.reshape(-1)[at].cpu().numpy(), golden["c_samples_f64"], float(golden["c_max_f64"]), float(golden["c_err"]))
    np.testing.assert_allclose(gm.center.cpu().numpy(), golden["c_center"], rtol=0, atol=1e-7)
    assert abs(gm.scale - float(golden["c_scale"])) <= 2e-7 * gm.scale


@pytest.mark.parametrize("name", ["single", "octant", "packed", "voxel_blocks"])
def test_edge_cases_against_float64(golden, name):
    cl, R, nb = field_inputs.edge_case(name)
    f64, info = _edge_reference(name)
    assert info["face_distance"] > 1e-5
    if name == "packed":
        assert info["members"].max() > 4096 and info["members"].max() % 256 != 0       # longer than the LDS list, ragged tail
    occ, _ = _kernel(cl, R, nb)
    ref_err = min(float(golden[n + "_err"]) for n in field_inputs.CASES)
    _check("edge_" + name, occ.cpu().numpy(), f64, np.abs(f64).max(), ref_err)
    s = R // nb
    empty = torch.from_numpy(np.repeat(np.repeat(np.repeat(info["members"] == 0, s, 0), s, 1), s, 2)).cuda()
    assert empty.any()
    assert (occ[empty] == 0).all()              # blocks without a member are exactly zero


@pytest.mark.parametrize("R,nb", sorted(field_inputs.LARGE_BLOCKS))
def test_large_blocks_against_float64(golden, R, nb):
    """4, 8 and 16 voxels per lane and the kernel's second pass (tests/field_inputs.py: LARGE_BLOCKS), under the edge cases' bar.  Every
    kept Gaussian is a member of every block here, so there is no empty block to assert on."""
    cl, R, nb = field_inputs.large_block_case(R, nb)
    f64, info = field_reference.density_field(cl["xyz"], cl["opacity"], cl["scaling"], cl["rotation"], R, nb)
    assert info["face_distance"] > 1e-5
    assert (R // nb) ** 3 > 512 and info["kept"] > 0 and (info["members"] == info["kept"]).all()
    occ, _ = _kernel(cl, R, nb)
    ref_err = min(float(golden[n + "_err"]) for n in field_inputs.CASES)
    _check("large_%d_%d" % (R, nb), occ.cpu().numpy(), f64, np.abs(f64).max(), ref_err)


def test_nothing_passes_the_prefilter():
    cl, R, nb = field_inputs.edge_case("transparent")
    occ, _ = _kernel(cl, R, nb)
    assert occ.shape == (R, R, R) and torch.equal(occ, torch.zeros_like(occ))


def test_bitwise_repeatable():
    cl, R, nb = field_inputs.edge_case("repeat")
    first, _ = _kernel(cl, R, nb)
    second, _ = _kernel(cl, R, nb)
    assert float(first.max()) > 0 and torch.equal(first, second)


def test_argument_errors():
    cl, _, _ = field_inputs.edge_case("single")
    with pytest.raises(ValueError, match="divide"):
        _model(cl).extract_fields(resolution=30, num_blocks=16)
