"""The projection of rendered views onto the texture atlas without a GPU (csrc/texture_project.hip, utils/texture.py): the
restatement's own float32 error and the margins of its "could flip" flags, the cap on flagged texels, what the parity scene must
contain, the C-ABI's declaration, binding, export and host-side argument checks, and the packed view table."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import texture_project_inputs as inputs
import texture_project_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ["parity"] + list(inputs.EXTREMES)


def _scene(name):
    return inputs.parity_scene() if name == "parity" else inputs.extreme_scene(name)


def _project(sc, two_sided, unpremultiply, dtype):
    return ref.project(sc["vertices"], sc["faces"], sc["T"], sc["views"], sc["images"], sc["vis_depth"], sc["depth_tolerance"],
                       two_sided=two_sided, unpremultiply=unpremultiply, dtype=dtype)


# ---------------------------------------------------------------------------------------------------------------- the restatement
def test_margins_cover_the_float32_error():
    """Every margin is at least 8 times the largest float32 - float64 deviation of its quantity over all scenes and flag combinations,
    the recorded deviations (inputs.MEASURED) are not below the measured ones, and on unflagged texels the float32 restatement takes
    every decision as the float64 one does."""
    worst = {}
    for name in SCENES:
        sc = _scene(name)
        for two_sided, unpremultiply in inputs.FLAG_COMBINATIONS:
            r64, r32 = (_project(sc, two_sided, unpremultiply, dt) for dt in (np.float64, np.float32))
            for key, val in ref.deviations(r32["run"], r64["run64"]).items():
                worst[key] = max(worst.get(key, 0.0), val)
            sure = r64["owned"] & ~r64["flagged"]
            assert np.array_equal(r32["count"][sure], r64["count"][sure]), (name, two_sided, unpremultiply)
            assert np.array_equal(r32["flagged"], r64["flagged"])                     # the flags do not depend on dtype
            for key in ("color_sum", "weight_sum"):
                mx = np.abs(r64[key]).max()
                err = np.abs(r32[key].astype(np.float64) - r64[key])[sure].max() / mx if mx > 0 else 0.0
                print("%s two_sided=%d unpremultiply=%d %s: float32 restatement %.3e" % (name, two_sided, unpremultiply, key, err))
                assert err < 1e-4
    margins = {"w": ref.MARGIN, "px": ref.MARGIN_PX, "depth": ref.MARGIN, "cos": ref.MARGIN, "alpha": ref.MARGIN_ALPHA}
    print("deviations %s, margins %s" % (worst, margins))
    for key, margin in margins.items():
        assert 8 * worst[key] <= margin, (key, worst[key], margin)
        assert worst[key] <= inputs.MEASURED[key], (key, worst[key])
    assert ref.MARGIN_PX >= 1e-4 and ref.MARGIN >= 2e-5 and ref.MARGIN_ALPHA >= 2e-5     # never below the starting margins


@pytest.mark.parametrize("name", SCENES)
def test_flagged_texels_stay_under_the_cap(name):
    sc = _scene(name)
    for two_sided, unpremultiply in inputs.FLAG_COMBINATIONS:
        r = _project(sc, two_sided, unpremultiply, np.float64)
        share = r["flagged"].sum() / r["owned"].sum()
        print("%s two_sided=%d unpremultiply=%d: %d of %d owned texels flagged" % (name, two_sided, unpremultiply, r["flagged"].sum(), r["owned"].sum()))
        assert share <= inputs.FLAG_CAP
        assert not r["flagged"][~r["owned"]].any()
        for key in ("color_sum", "weight_sum", "count"):
            assert not r[key][~r["owned"]].any()


def parity_scene_content(r, sc):
    """What the parity scene must contain, from a float64 run of the restatement (two_sided=True)."""
    run = r["run64"]
    q, reached = run["q"], run["reached"]
    with np.errstate(all="ignore"):
        inside = reached[:, 1] & (q["sx"] >= 0) & (q["sx"] < sc["W"]) & (q["sy"] >= 0) & (q["sy"] < sc["H"])
    found = {"behind the camera": (reached[:, 0] & ~reached[:, 1]).any(), "off-screen": (reached[:, 1] & ~inside).any(),
             "empty pixel": (inside & ~reached[:, 2]).any(), "occluded": (reached[:, 2] & ~reached[:, 3]).any(),
             "below min_cos": (reached[:, 3] & ~reached[:, 4]).any(), "above min_cos": reached[:, 4].any(),
             "below min_alpha": (reached[:, 4] & ~reached[:, 5]).any(), "passing": reached[:, 5].any(),
             "degenerate face": (~run["live"]).any() and not run["count"][~run["live"]].any()}
    seen = np.bincount(r["count"][r["owned"]], minlength=4)
    return found, seen


def test_parity_scene_contents():
    sc = inputs.parity_scene()
    assert ref.texture_reference.layout(len(sc["faces"]), sc["T"])[0] == 12 and sc["K"] == 3 and (sc["H"], sc["W"]) == (45, 67)
    r = _project(sc, True, False, np.float64)
    assert r["owned"].sum() == 2880
    found, seen = parity_scene_content(r, sc)
    assert all(found.values()), found
    assert len(seen) == 4 and (seen > 0).all(), seen                   # texels seen by 0, 1, 2 and 3 views
    assert (r["run64"]["face"][~r["run64"]["live"]] == inputs.DEGENERATE).all()
    # the sheet hides something in view 0 that is visible without it
    bare = inputs._finish(sc["vertices"], sc["faces"], sc["T"], list(zip(sc["projs"], sc["centres"])), sc["images"], sc["depth_tolerance"])
    r0 = ref.project(sc["vertices"], sc["faces"], sc["T"], sc["views"], sc["images"], bare["vis_depth"], sc["depth_tolerance"])
    assert r0["count"].sum() > r["count"].sum()


# ---------------------------------------------------------------------------------------------------------------- C-ABI
def test_symbol_declared_bound_and_exported():
    from gaussianip_amd import _lib
    assert _lib.TEXTURE_PROJECT_SYMBOLS == ["gip_texture_project"]
    header = open(os.path.join(ROOT, "include", "gip_model.h")).read()
    so = os.path.join(_lib.LIB_DIR, "libgip_model.so")
    names = {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout.splitlines()
             if ln.strip()}
    for sym in _lib.TEXTURE_PROJECT_SYMBOLS:
        assert re.search(r"\bint %s\(" % sym, header) and sym in names, sym
    assert len(_lib.model_lib()._lib.gip_texture_project.argtypes) == 21
    makefile = open(os.path.join(ROOT, "gaussianip_amd", "csrc", "Makefile")).read()
    assert makefile.count("texture_project.hip") == 2 and "-ffp-contract=off" in makefile


def test_entry_point_argument_checks_launch_nothing():
    from gaussianip_amd import _lib
    bound = _lib.model_lib()

    def call(V=30, F=10, T=64, cell=8, K=3, H=45, W=67, min_alpha=0.5, unpremultiply=0, ptr=None, images=None):
        """Every array NULL, or the non-NULL dummy `ptr`, which nothing may dereference."""
        return bound.gip_texture_project(ptr, V, ptr, F, T, cell, K, ptr, images if images is not None else ptr, ptr, H, W, 0.01, 0.2, min_alpha,
                                         1, unpremultiply, ptr, ptr, ptr, None)
    assert call(F=0) == 0                                    # no faces: a successful no-op
    assert call() == 1                                       # faces without their arrays
    assert call(K=0, F=0) == 1 and call(K=65, F=0) == 1 and call(K=-1, F=0) == 1
    assert call(K=64, F=0) == 0 and call(K=1, F=0) == 0
    assert call(T=3, cell=3, F=0) == 1 and call(T=16385, F=0) == 1
    assert call(cell=3, F=0) == 1 and call(T=64, cell=65, F=0) == 1
    assert call(T=64, cell=8, F=129) == 1                    # 2 (T // cell)^2 = 128 < F
    assert call(T=64, cell=8, F=128) == 1                    # fits, but the arrays are NULL
    assert call(H=0, F=0) == 1 and call(W=16385, F=0) == 1
    assert call(F=2 ** 31) == 1 and call(V=2 ** 31, F=0) == 1 and call(F=-1) == 1 and call(V=-1, F=0) == 1
    assert call(unpremultiply=1, min_alpha=0.0, F=0) == 1 and call(unpremultiply=1, min_alpha=0.5, F=0) == 0
    dummy = ctypes.c_void_p(64)
    assert call(ptr=dummy, V=0) == 1                         # faces without vertices
    assert call(ptr=dummy, images=ctypes.c_void_p(68)) == 1  # images not 16-byte aligned


# ---------------------------------------------------------------------------------------------------------------- host side
def _cam(M, centre, h=inputs.H, w=inputs.W):
    return types.SimpleNamespace(full_proj_transform=torch.from_numpy(np.asarray(M, np.float32)), camera_center=torch.from_numpy(np.asarray(centre, np.float32)),
                                 image_height=h, image_width=w)


def test_view_table_of_one_camera():
    """pack_views against a table written out by hand for a Camera of the project: 16 values of full_proj_transform row by row,
    the camera centre, a zero."""
    import math

    from gaussianip_amd.scene import Camera
    from gaussianip_amd.utils import texture as tex
    c2w = torch.eye(4)
    c2w[:3, 3] = torch.tensor([0.5, -0.25, 2.0])
    cam = Camera(c2w=c2w, FoVy=math.radians(50.0), height=45, width=67, data_device="cpu")
    table = tex.pack_views([cam])
    assert table.shape == (1, 20) and table.dtype == torch.float32 and table.is_contiguous()
    want = np.zeros(20, np.float32)
    full = cam.full_proj_transform.numpy()
    for i in range(4):
        for j in range(4):
            want[4 * i + j] = full[i, j]
    want[16], want[17], want[18] = (float(x) for x in cam.camera_center)
    assert np.array_equal(table[0].numpy(), want) and want[19] == 0
    # the convention: the camera's own centre projects to w = 0, and a point in front of it to w > 0
    centre = np.append(cam.camera_center.numpy().astype(np.float64), 1.0)
    assert abs(centre @ full.astype(np.float64)[:, 3]) < 1e-6
    # the restatement's packing is the same table
    assert np.array_equal(ref.pack_views([full], [cam.camera_center.numpy()])[0], want)
    two = tex.pack_views([cam, _cam(np.eye(4), [1, 2, 3])])
    assert two.shape == (2, 20) and np.array_equal(two[1].numpy(), np.concatenate((np.eye(4).ravel(), [1, 2, 3, 0])).astype(np.float32))


def test_host_side_validation_needs_no_gpu():
    from gaussianip_amd import _lib
    from gaussianip_amd.scene import GaussianModel
    from gaussianip_amd.utils import texture as tex
    before = _lib.call_counts.get("gip_texture_project", 0)
    v, f = torch.zeros((6, 3)), torch.zeros((2, 3), dtype=torch.int32)
    cam = _cam(np.eye(4), [0, 0, 0])
    img, vis = torch.zeros((1, 3, inputs.H, inputs.W)), torch.zeros((1, inputs.H, inputs.W))
    with pytest.raises(ValueError, match="1 .. 64"):
        tex.project_views(v, f, 16, [], img, vis, depth_tolerance=0.1)
    with pytest.raises(ValueError, match="1 .. 64"):
        tex.project_views(v, f, 16, [cam] * 65, img, vis, depth_tolerance=0.1)
    with pytest.raises(ValueError, match="1 .. 64"):
        tex.visible_depth([], v, f)
    with pytest.raises(ValueError, match="image size"):
        tex.project_views(v, f, 16, [cam, _cam(np.eye(4), [0, 0, 0], h=44)], img, vis, depth_tolerance=0.1)
    with pytest.raises(ValueError, match="min_alpha"):
        tex.project_views(v, f, 16, [cam], img, vis, depth_tolerance=0.1, unpremultiply=True, min_alpha=0.0)
    with pytest.raises(ValueError, match="depth_tolerance"):
        tex.project_views(v, f, 16, [cam], img, vis, depth_tolerance=-1.0)
    with pytest.raises(ValueError, match="GPU"):                 # tensors on the CPU
        tex.project_views(v, f, 16, [cam], img, vis, depth_tolerance=0.1)
    with pytest.raises(ValueError, match="GPU"):
        tex.visible_depth([cam], v, f)
    gm = GaussianModel(0)
    with pytest.raises(ValueError, match="cameras"):
        gm.extract_textured_mesh(bake="views")
    with pytest.raises(ValueError, match="bake"):
        gm.extract_textured_mesh(bake="images")
    with pytest.raises(ValueError, match="bake='views'"):
        gm.extract_textured_mesh(cameras=[cam])
    with pytest.raises(ValueError, match="1 .. 64"):
        gm.bake_texture_from_views(v, f, [cam] * 65, None)
    with pytest.raises(ValueError, match="min_alpha"):
        gm.bake_texture_from_views(v, f, [cam], None, min_alpha=0.0)      # images=None: unpremultiply is on
    assert _lib.call_counts.get("gip_texture_project", 0) == before
