"""Pixel differentials and the mipmapped lookup without a GPU (csrc/mesh_mip.hip, tests/mesh_mip_reference.py): the exported symbols,
the host's level count, the float64 restatement's analytic pieces against central differences (tests/test_mesh_grad_cpu.py's
_richardson: two step sizes, the bar at 4 times their difference), and the fold as the exact transpose of the build."""
import ctypes
import os
import subprocess

import numpy as np

import mesh_grad_inputs as scenes
import mesh_mip_reference as mref
import mesh_render_reference as ref
from test_mesh_grad_cpu import _richardson

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 13, 19
F64 = np.float64


def test_symbols_exported():
    from gaussianip_amd import _lib
    assert len(_lib.MESH_MIP_SYMBOLS) == 8 and len(set(_lib.MESH_MIP_SYMBOLS)) == 8
    assert not set(_lib.MESH_MIP_SYMBOLS) & (set(_lib.MESH_SYMBOLS) | set(_lib.MESH_GRAD_SYMBOLS))
    so = os.path.join(ROOT, "gaussianip_amd", "lib", "libgip_model.so")
    assert os.path.exists(so), "libgip_model.so is not built"
    names = {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout.splitlines()
             if ln.strip()}
    lib = _lib.model_lib()
    with open(os.path.join(ROOT, "include", "gip_model.h")) as fh:
        header = fh.read()
    for sym in _lib.MESH_MIP_SYMBOLS:
        assert sym in names, sym
        assert getattr(lib, sym) is not None
        assert "int %s(" % sym in header, sym


def test_level_count_of_the_host():
    from gaussianip_amd import _lib
    lib = _lib.model_lib()
    cases = [(16, 8, None), (12, 20, None), (1, 8, None), (7, 7, None), (16, 16, 1), (16, 16, 0), (1, 1, None), (4096, 4096, None),
             (16384, 2, None), (6, 1, None), (64, 64, 3), (1024, 48, None), (2, 2, 5)]
    for Th, Tw, cap in cases:
        L, texels = ctypes.c_int32(-1), ctypes.c_int64(-1)
        assert lib.gip_mesh_mip_levels(Th, Tw, -1 if cap is None else cap, ctypes.byref(L), ctypes.byref(texels)) == 0
        want = mref.mip_levels(Th, Tw, cap)
        sides = [(max(Th >> l, 1), max(Tw >> l, 1)) for l in range(1, want + 1)]
        assert L.value == want and texels.value == sum(h * w for h, w in sides), (Th, Tw, cap, L.value, want)
    assert [mref.mip_levels(*c) for c in cases[:5]] == [4, 2, 3, 0, 1]
    assert [t.shape[:2] for t in mref.mip_build(np.zeros((12, 20, 2)), None, F64)] == [(12, 20), (6, 10), (3, 5)]
    assert lib.gip_mesh_mip_levels(0, 4, -1, ctypes.byref(L), ctypes.byref(texels)) == 1
    assert lib.gip_mesh_mip_levels(4, 20000, -1, ctypes.byref(L), ctypes.byref(texels)) == 1


def _scene(view=0):
    """One view of the silhouette scene at 13 x 19; view 1 has w spread over 1 .. 20, so (u, v) is far from linear in the pixel."""
    pos, tri = scenes.silhouette_views(B=2)
    pos, _, _ = scenes.on_the_grid(pos[view:view + 1], H, W)
    ids = ref.rasterize(pos, tri, H, W)["tri"]
    u, v, _ = ref.barycentrics(pos, tri, H, W, ids, F64)
    return pos, tri, ids, u, v


def test_rast_db_against_differences():
    """rast_db is the derivative of the restated (u, v) in the pixel position, the triangle held fixed.  Under the strong perspective
    of view 1 the differences' truncation error, not their rounding, sets the bar."""
    pos, tri, ids, u, v = _scene(1)
    db = mref.rast_db(pos, tri, H, W, ids, u, v, F64)
    assert not db[ids < 0].any() and (ids < 0).sum() > 20
    py, px = np.nonzero(ids[0] >= 0)
    pick = np.random.default_rng(3).choice(len(py), 24, replace=False)
    py, px = py[pick], px[pick]
    assert len(np.unique(ids[0, py, px])) >= 4
    g = np.random.default_rng(4).normal(size=(len(py), 2))
    for n in range(len(py)):      # the restatement at the pixel centre is rast's (u, v)
        assert np.allclose(mref.uv_at(pos[0], tri[ids[0, py[n], px[n]]], H, W, (px[n], py[n])), (u[0, py[n], px[n]], v[0, py[n], px[n]]), rtol=0, atol=1e-14)

    def loss(points):
        return float(sum((g[n] * mref.uv_at(pos[0], tri[ids[0, py[n], px[n]]], H, W, points[n])).sum() for n in range(len(py))))

    d = db[0, py, px]
    analytic = np.stack((g[:, 0] * d[:, 0] + g[:, 1] * d[:, 2], g[:, 0] * d[:, 1] + g[:, 1] * d[:, 3]), 1)
    _richardson("rast_db", analytic, loss, np.stack((px, py), 1).astype(F64))


def test_out_da_gradient_against_differences():
    pos, tri, ids, u, v = _scene()
    db = mref.rast_db(pos, tri, H, W, ids, u, v, F64)
    rng = np.random.default_rng(5)
    attr = rng.normal(size=(pos.shape[1], 3))
    g = rng.normal(size=(1, H, W, 4))
    analytic = mref.interpolate_da_grad(attr.shape, tri, ids, db, [2, 0], g, F64)
    assert not analytic[:, 1].any()                                     # the channel that is not listed
    _richardson("out_da to attr", analytic, lambda a: float((g * mref.interpolate_da(a, tri, ids, db, [2, 0], F64)).sum()), attr)
    # out_da is what the differences of the interpolated attribute give: the definition's da/dX against interpolate at shifted (u, v)
    out_da = mref.interpolate_da(attr, tri, ids, db, None, F64)
    cov = ids >= 0
    h = 1e-5
    for axis in (0, 1):
        hi = ref.interpolate(attr, tri, ids, u + h * db[..., axis], v + h * db[..., 2 + axis], F64)
        lo = ref.interpolate(attr, tri, ids, u - h * db[..., axis], v - h * db[..., 2 + axis], F64)
        assert np.abs((hi - lo) / (2 * h) - out_da[..., axis::2])[cov].max() <= 1e-9 * np.abs(out_da).max()


def _lookup_case():
    """A 16 x 16 x 3 stack (L = 4) and 40 pixels whose levels lie in [0.3, 3.7] with a fractional part in [0.2, 0.8] and whose bilinear
    fractions at both levels lie in [0.1, 0.9]: away from every kink by far more than the steps move them."""
    rng = np.random.default_rng(6)
    levels = mref.mip_build(rng.normal(size=(16, 16, 3)), None, F64)
    n = 4000
    uv = rng.uniform(-0.2, 1.2, (n, 2))
    target = rng.integers(0, 4, n) + rng.uniform(0.3, 0.7, n)
    major, minor, phi = 2.0 ** target / 16, rng.uniform(0.3, 1.0, n), rng.uniform(0, 2 * np.pi, n)
    rot = np.stack((np.cos(phi), -np.sin(phi), np.sin(phi), np.cos(phi)), -1).reshape(n, 2, 2)
    jac = rot @ (np.stack((major, major * minor), -1)[:, :, None] * np.eye(2))      # columns: the ellipse's axes in uv
    uv_da = np.stack((jac[:, 0, 0], jac[:, 0, 1], jac[:, 1, 0], jac[:, 1, 1]), -1)
    bias = rng.uniform(-0.1, 0.1, n)
    level = mref.lod(uv_da, bias, 16, 16, (n,), F64)["level"]
    assert np.abs(level - (target + bias)).max() < 1e-9                 # the major axis sets the level
    keep = (np.abs(level - np.rint(level)) > 0.2) & (level > 0.3) & (level < 3.7)
    l0 = np.floor(level).astype(int)
    for k in (0, 1):
        side = 16 / 2.0 ** (l0 + k)
        for axis in (0, 1):
            frac = (uv[:, axis] * side - 0.5) % 1.0
            keep &= (frac > 0.1) & (frac < 0.9)
    idx = np.nonzero(keep)[0][:40]
    assert len(idx) == 40 and len(np.unique(l0[idx])) == 4
    return levels, uv[idx], uv_da[idx], bias[idx], rng.normal(size=(40, 3))


def test_texture_gradients_against_differences():
    levels, uv, uv_da, bias, g = _lookup_case()
    _, g_uv, g_da, g_bias, _ = mref.texture_mip_grad(levels, uv, uv_da, bias, g, F64)
    _richardson("texture to uv", g_uv, lambda x: float((g * mref.texture_mip(levels, x, uv_da, bias, F64)).sum()), uv)
    _richardson("texture to uv_da", g_da, lambda x: float((g * mref.texture_mip(levels, uv, x, bias, F64)).sum()), uv_da)
    _richardson("texture to bias", g_bias, lambda x: float((g * mref.texture_mip(levels, uv, uv_da, x, F64)).sum()), bias)
    # the gradient to the texture through a random direction (the lookup is linear in it)
    d = np.random.default_rng(7).normal(size=levels[0].shape)
    g_tex = mref.texture_mip_grad(levels, uv, uv_da, bias, g, F64)[0]
    moved = mref.mip_build(levels[0] + d, None, F64)
    lhs = float((g * (mref.texture_mip(moved, uv, uv_da, bias, F64) - mref.texture_mip(levels, uv, uv_da, bias, F64))).sum())
    assert abs(lhs - float((g_tex * d).sum())) <= 1e-12 * np.abs(g_tex).sum()
    # the degenerate ellipse: a square root of 0 takes dm/dA = dm/dB = 0.5, dm/dC = 0, and m = 0 gives no gradient
    iso = np.tile(np.array([[0.2, 0.0, 0.0, 0.2]]), (2, 1))
    iso[1] = 0
    _, _, g_iso, _, _ = mref.texture_mip_grad(levels, uv[:2], iso, None, g[:2], F64)
    assert np.isfinite(g_iso).all() and g_iso[0, 0] != 0 and g_iso[0, 1] == 0 and not g_iso[1].any()


def test_the_fold_is_the_transpose_of_the_build():
    rng = np.random.default_rng(8)
    for shape, cap in (((16, 8, 3), None), ((12, 20, 2), None), ((1, 8, 1), None), ((7, 7, 3), None), ((16, 16, 3), 1), ((32, 2, 1), None)):
        x = rng.normal(size=shape)
        built = mref.mip_build(x, cap, F64)
        y = [rng.normal(size=t.shape) for t in built]
        lhs = sum(float((a * b).sum()) for a, b in zip(built, y))
        rhs = float((x * mref.mip_fold(y, F64)).sum())
        scale = sum(float(np.abs(a * b).sum()) for a, b in zip(built, y))
        assert abs(lhs - rhs) <= 1e-13 * scale, (shape, lhs, rhs)
        assert len(built) - 1 == mref.mip_levels(shape[0], shape[1], cap)
        # float32 build: the same additions in the same order as float64 rounded once per operation
        b32 = mref.mip_build(x.astype(np.float32), cap, np.float32)
        assert all(t.dtype == np.float32 for t in b32)
