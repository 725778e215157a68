"""The density field without a GPU: tests/field_reference.py (the definition restated in float64 numpy) against the reference's own
numbers in tests/golden/field.npz (tools/make_golden.py group `field`), the C-ABI's declarations, bindings and exports, and the
argument check of GaussianModel.extract_fields.

field_reference reproduces the reference's float64 samples of case c to 1e-12 of the field's maximum, and lies within the
reference's own float32 error (the stored `err`) plus 1e-7, both relative to the maximum, of its float32 fields: the fixture and
the restatement check each other, and the GPU tests may take the restatement as their float64 side."""
import ctypes
import os
import re

import numpy as np
import pytest

import field_inputs
import field_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return field_inputs.load_golden()


def _reference(name, voxels=None):
    cl, R, nb = field_inputs.case(name)
    return field_reference.density_field(cl["xyz"], cl["opacity"], cl["scaling"], cl["rotation"], R, nb, voxels=voxels)


def test_stored_errors_keep_the_bar_discriminating(golden):
    for name in field_inputs.CASES:
        assert 0 < float(golden[name + "_err"]) <= 1e-4


@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_matches_float32_fields(golden, name):
    f64, info = _reference(name)
    mx = np.abs(f64).max()
    assert abs(mx - float(golden[name + "_max_f64"])) <= 1e-12 * mx
    got = np.abs(golden[name + "_field"].astype(np.float64) - f64).max() / mx
    print("case %s: restatement vs float32 fixture %.3e, stored err %.3e" % (name, got, float(golden[name + "_err"])))
    assert got <= float(golden[name + "_err"]) + 1e-7
    assert info["face_distance"] > 1e-5
    np.testing.assert_allclose(info["center"], golden[name + "_center"], rtol=0, atol=1e-6)
    assert abs(info["scale"] - float(golden[name + "_scale"])) <= 1e-6 * info["scale"]


def test_restatement_matches_float64_samples(golden):
    at = field_inputs.sample_voxels(field_inputs.CASES["c"][1])
    f64, info = _reference("c", voxels=at)
    mx = float(golden["c_max_f64"])
    assert np.count_nonzero(golden["c_samples_f64"]) > 1000
    assert np.abs(f64 - golden["c_samples_f64"]).max() <= 1e-12 * mx
    assert np.abs(golden["c_samples_f32"].astype(np.float64) - f64).max() / mx <= float(golden["c_err"]) + 1e-7
    assert info["face_distance"] > 1e-5


def test_symbols_declared_bound_and_exported():
    from gaussianip_amd import _lib
    header = open(os.path.join(ROOT, "include", "gip_model.h")).read()
    assert _lib.FIELD_SYMBOLS == ["gip_field_workspace_size", "gip_density_field", "gip_surface_count", "gip_surface_emit"]
    lib = ctypes.CDLL(os.path.join(_lib.LIB_DIR, "libgip_model.so"))
    for sym in _lib.FIELD_SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, header), sym
        getattr(lib, sym)
    bound = _lib.model_lib()
    need = ctypes.c_size_t(0)
    assert bound.gip_field_workspace_size(1000, 128, 16, ctypes.byref(need)) == 0 and need.value == 1000 * 48
    assert bound.gip_field_workspace_size(1000, 30, 16, ctypes.byref(need)) == 1       # num_blocks does not divide the resolution
    assert bound.gip_field_workspace_size(-1, 32, 8, ctypes.byref(need)) == 1
    assert bound.gip_surface_count(None, 8, 0.0, None, None, None) == 1                # NULL pointers: nothing is launched


def test_extract_fields_rejects_indivisible_resolution():
    from gaussianip_amd.scene import GaussianModel
    with pytest.raises(ValueError, match="divide"):
        GaussianModel(0, device="cpu").extract_fields(resolution=30, num_blocks=16)
