"""The mesh rasterizer without a GPU: the exported symbols, the watertightness of the definition as tests/mesh_render_reference.py
restates it, and the argument checks that need no device."""
import os
import subprocess

import numpy as np
import pytest
import torch

import mesh_render_inputs as inputs
import mesh_render_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_exported():
    from gaussianip_amd import _lib
    assert _lib.TEXTURE_SYMBOLS == ["gip_texture_bake_workspace_size", "gip_texture_bake"]
    assert _lib.MESH_SYMBOLS == ["gip_mesh_raster_workspace_size", "gip_mesh_rasterize", "gip_mesh_interpolate",
                                 "gip_mesh_interpolate_backward", "gip_mesh_texture", "gip_mesh_texture_backward", "gip_mesh_shade",
                                 "gip_mesh_shade_backward"]
    so = os.path.join(ROOT, "gaussianip_amd", "lib", "libgip_model.so")
    assert os.path.exists(so), "libgip_model.so is not built"
    names = {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout.splitlines()
             if ln.strip()}
    for sym in _lib.MESH_SYMBOLS + _lib.TEXTURE_SYMBOLS:
        assert sym in names, sym


def test_workspace_size_formula():
    """utils.rasterize sizes the workspace with the library's formula without asking it (a render is two calls into the library)."""
    import ctypes
    from gaussianip_amd import _lib
    from gaussianip_amd.utils import rasterize
    lib = _lib.model_lib()
    for B, h, w, F in ((1, 1, 1, 1), (2, 45, 67, 331), (4, 1024, 1024, 1741484), (16, 16384, 8191, 2 ** 24 - 1)):
        size = ctypes.c_size_t(0)
        assert lib.gip_mesh_raster_workspace_size(B, h, w, F, ctypes.byref(size)) == 0
        assert size.value == rasterize._workspace_bytes(B, h, w, F)
    for B, h, w, F in ((0, 8, 8, 1), (1, 16385, 8, 1), (1, 8, 8, 2 ** 24), (17, 16384, 8192, 1)):
        assert lib.gip_mesh_raster_workspace_size(B, h, w, F, ctypes.byref(ctypes.c_size_t(0))) == 1


@pytest.mark.parametrize("on_centres", [False, True])
def test_the_definition_is_watertight(on_centres):
    """Every pixel of a triangulated grid that covers the image is covered by exactly one triangle: shared edges and shared vertices
    have one owner, whatever the windings, also when vertices lie exactly on pixel centres."""
    pos, tri = inputs.grid_mesh(3, on_centres=on_centres)
    X, Y, ok = ref.snap(pos, inputs.H, inputs.W)
    assert ok.all()
    if on_centres:
        assert (X % 256 == 128).all() and (Y % 256 == 128).all()
        inside = (X > 0) & (X < 256 * inputs.W) & (Y > 0) & (Y < 256 * inputs.H)
        assert inside.sum() >= 30                                 # pixel centres that are shared vertices, inside the image
    out = ref.rasterize(pos[None], tri, inputs.H, inputs.W)
    assert (out["covering"] == 1).all()
    assert (out["tri"] >= 0).all()
    areas = [ref._setup(X, Y, ok, t)[6] for t in tri]
    assert min(areas) < 0 < max(areas)                            # both windings
    culled = ref.rasterize(pos[None], tri, inputs.H, inputs.W, cull_backfaces=True)
    assert ((culled["covering"] == 1) == (np.array(areas)[out["tri"]] > 0)).all()


def test_the_scene_holds_what_it_promises():
    pos, tri, tags = inputs.coverage_views()
    out = ref.rasterize(pos, tri, inputs.H, inputs.W)
    X, Y, ok = ref.snap(pos, inputs.H, inputs.W)
    won = set(np.unique(out["tri"]))
    for name in ("zero_area", "behind", "guard_band", "subpixel"):
        assert not won & set(tags[name]), name
    assert ok[0][tri[tags["zero_area"][0]]].all() and not ok[0][tri[tags["guard_band"][0]]].all()
    assert tags["depth_out"][0] not in won and tags["depth_out"][1] in won and tags["depth_out"][2] in won
    assert tags["coincident"][0] in won and tags["coincident"][1] not in won
    assert all(t in won for t in tags["screen_filling"])            # they interpenetrate: each wins somewhere
    assert len(won & set(tags["random"])) > 20
    box = [X[0][tri[tags["random"]]].min(1), X[0][tri[tags["random"]]].max(1)]
    assert ((box[1] < 0) | (box[0] > 256 * inputs.W)).any() and ((box[0] < 0) & (box[1] > 0)).any()      # wholly and partly off-screen


def test_cpu_tensors_are_refused():
    from gaussianip_amd.utils.rasterize import MeshRasterizerContext, render_mesh
    ctx = MeshRasterizerContext()
    pos, tri = inputs.grid_mesh(3)
    with pytest.raises(ValueError):
        ctx.rasterize(torch.from_numpy(pos)[None], torch.from_numpy(tri), (inputs.H, inputs.W))
    with pytest.raises(ValueError):
        ctx.interpolate(torch.zeros(63, 5), torch.zeros(1, 4, 4, 4), torch.from_numpy(tri))
    with pytest.raises(ValueError):
        ctx.texture(torch.zeros(1, 4, 4, 3), torch.zeros(1, 4, 4, 2))
    with pytest.raises(NotImplementedError):
        ctx.antialias(None, None, None, None)

    class Cam:
        image_height, image_width = inputs.H, inputs.W
        full_proj_transform = torch.from_numpy(inputs.EXACT_PROJ)
    with pytest.raises(ValueError):
        render_mesh(Cam(), torch.from_numpy(inputs.world_of(pos)), torch.from_numpy(tri), torch.zeros(len(tri), 3, 2),
                    torch.zeros(8, 8, 3))
