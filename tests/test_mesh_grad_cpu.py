"""Gradients to vertex positions and the antialias pass without a GPU (csrc/mesh_grad.hip, tests/mesh_grad_reference.py): the exported
symbols, edge_topology against a brute-force count, the restatement's analytic gradients against central differences, and the exact
row sums of an antialiased rectangle.

The difference tests run the restatement in float64 with snapping switched off (float64 screen coordinates, the integer decisions of
the base point held fixed), on a scene whose vertices lie on the sub-pixel grid and that has no ties.  Their bar is not a fixed
number: central differences are taken at steps h and h / 2, whose mutual difference estimates the truncation error (Richardson), and
the analytic gradient must agree with the finer one to 4 times that."""
import os
import subprocess

import numpy as np
import torch

import mesh_grad_inputs as scenes
import mesh_grad_reference as gref
import mesh_render_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 13, 19
STEP = 1e-4


def test_symbols_exported():
    from gaussianip_amd import _lib
    assert _lib.MESH_GRAD_SYMBOLS == ["gip_mesh_rasterize_backward", "gip_mesh_interpolate_backward_rast", "gip_mesh_shade_backward_rast",
                                      "gip_mesh_antialias", "gip_mesh_antialias_backward"]
    assert len(_lib.MESH_SYMBOLS) == 8 and not set(_lib.MESH_SYMBOLS) & set(_lib.MESH_GRAD_SYMBOLS)
    so = os.path.join(ROOT, "gaussianip_amd", "lib", "libgip_model.so")
    assert os.path.exists(so), "libgip_model.so is not built"
    names = {ln.split()[-1] for ln in subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout.splitlines()
             if ln.strip()}
    for sym in _lib.MESH_GRAD_SYMBOLS:
        assert sym in names, sym
    lib = _lib.model_lib()
    for sym in _lib.MESH_GRAD_SYMBOLS:
        assert getattr(lib, sym) is not None
    with open(os.path.join(ROOT, "include", "gip_model.h")) as fh:
        header = fh.read()
    for sym in _lib.MESH_GRAD_SYMBOLS:
        assert "int %s(" % sym in header, sym


def test_edge_topology_against_a_count():
    from gaussianip_amd.utils.rasterize import edge_topology
    # a strip of four faces with both windings (boundary and regular interior edges), and two more faces on the edge (0, 1)
    tri = np.array([[0, 1, 2], [2, 1, 3], [3, 4, 2], [4, 3, 5], [1, 0, 6], [0, 1, 7]], np.int32)
    want = gref.edge_topology(tri)
    assert (want == -1).any() and (want == -2).sum() == 3 and (want >= 0).sum() == 6
    got = edge_topology(torch.from_numpy(tri), 8)
    assert got.dtype == torch.int32 and got.shape == (6, 3) and not got.is_cuda
    assert np.array_equal(got.numpy(), want)
    assert want[0, 0] == 3 and want[1, 2] == 0          # the edge (1, 2) seen from both faces, whatever their windings
    # the scene of the GPU tests: the fold's shared edge names the other face's corner, the three-face edge reads -2
    want = gref.edge_topology(scenes.TRI)
    assert np.array_equal(edge_topology(torch.from_numpy(scenes.TRI), 17).numpy(), want)
    assert want[4, 2] == 11 and want[5, 2] == 10 and (want[6:, 2] == -2).all() and want[0, 1] == 3 and want[0, 0] == -1
    assert edge_topology(torch.zeros((0, 3), dtype=torch.int32), 4).shape == (0, 3)
    # a random closed surface (an octahedron): every edge regular
    octa = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    got = edge_topology(torch.from_numpy(octa), 6).numpy()
    assert np.array_equal(got, gref.edge_topology(octa)) and (got >= 0).all()


def _scene():
    """One view of the silhouette scene at 13 x 19 with its vertices on the sub-pixel grid; asserts, in integers, that it has no ties."""
    pos, tri = scenes.silhouette_views(B=1)
    pos, X, Y = scenes.on_the_grid(pos, H, W)
    out = ref.rasterize(pos, tri, H, W)
    ids, depth = out["tri"], out["depth"]
    py, px = np.mgrid[0:H, 0:W].astype(np.int64)
    for t in tri:                                           # no edge passes through a pixel centre
        s = ref._setup(X[0], Y[0], np.ones(len(X[0]), bool), t)
        e0, e1, e2, _ = ref._edges(s, 256 * px + 128, 256 * py + 128)
        assert (e0 != 0).all() and (e1 != 0).all() and (e2 != 0).all()
    topo = gref.edge_topology(tri)
    hits = gref.antialias_hits(pos, tri, topo, ids, depth, H, W)
    for h in hits:                                          # no tau is 0 or 256, nor 128 (where the blend changes its target)
        assert 0 < h["n"] < 256 * h["D"] and 2 * h["n"] != 256 * h["D"]
    return pos.astype(np.float64), tri, ids, depth, topo, hits


def _differences(f, x, step):
    g = np.zeros_like(x)
    for i in np.ndindex(*x.shape):
        hi, lo = x.copy(), x.copy()
        hi[i] += step
        lo[i] -= step
        g[i] = (f(hi) - f(lo)) / (2 * step)
    return g


def _richardson(name, analytic, f, x):
    coarse, fine = _differences(f, x, STEP), _differences(f, x, STEP / 2)
    bar = 4 * np.abs(coarse - fine).max()
    err = np.abs(analytic - fine).max()
    print("%s: |analytic - differences| %.3e, bar %.3e (4 x the difference between steps %g and %g), gradient maximum %.3e" % (
        name, err, bar, STEP, STEP / 2, np.abs(fine).max()))
    assert np.abs(fine).max() > 1e-2 and bar < 1e-3 * np.abs(fine).max()       # the gradient is there and the bar resolves it
    assert err <= bar, (name, err, bar)


def test_rasterize_backward_against_differences():
    pos, tri, ids, _, _, _ = _scene()
    assert len(np.unique(ids)) >= 8 and (ids < 0).sum() > 20
    g = np.random.default_rng(1).normal(size=(1, H, W, 4))

    def loss(p):
        u, v, d = gref.rasterize_values(p, tri, H, W, ids, np.float64, snapped=False)
        return float((g[..., 0] * u + g[..., 1] * v + g[..., 2] * d).sum())

    analytic = gref.rasterize_grad(pos, tri, H, W, ids, g, np.float64, snapped=False)
    assert np.abs(analytic[..., 3]).max() > 0.1 and np.abs(analytic[..., 2]).max() > 0.1
    _richardson("rasterize backward", analytic, loss, pos)
    # on the grid, snapping changes nothing but the last bits
    snapped = gref.rasterize_grad(pos, tri, H, W, ids, g, np.float64, snapped=True)
    assert np.abs(snapped - analytic).max() <= 1e-4 * np.abs(analytic).max()


def test_antialias_backward_against_differences():
    pos, tri, ids, depth, topo, hits = _scene()
    kinds = {(h["face"], h["edge"]) for h in hits}
    assert len(hits) > 60 and {h["axis"] for h in hits} == {0, 1} and {h["s"] for h in hits} == {-1, 1}
    assert any(h["face"] in scenes.TAGS["fold"] and h["edge"] == 2 for h in hits)          # the folded edge blends
    assert not any(h["face"] in scenes.TAGS["three"] and h["edge"] == 2 for h in hits)     # the three-face edge never does
    assert not any(h["face"] in (0, 2) and h["edge"] == 1 for h in hits) and len(kinds) > 10      # nor a quad's diagonal
    rng = np.random.default_rng(2)
    color = rng.uniform(0, 1, (1, H, W, 3)) * (ids >= 0)[..., None] + rng.uniform(0, 0.2, (1, H, W, 3))
    g = rng.normal(size=(1, H, W, 3))
    out = gref.antialias(color, hits, pos, H, W, np.float64, snapped=False)
    changed = np.abs(out - color).max(-1) > 0
    assert 40 < changed.sum() < H * W // 2
    g_color, g_pos = gref.antialias_grad(color, hits, pos, g, H, W, np.float64, snapped=False)
    _richardson("antialias backward, pos", g_pos, lambda p: float((g * gref.antialias(color, hits, p, H, W, np.float64, snapped=False)).sum()), pos)
    # linear in color: the differences are exact up to rounding, so the gradient is compared through a random direction
    d = rng.normal(size=color.shape)
    lhs = float((g * (gref.antialias(color + d, hits, pos, H, W, np.float64, False) - out)).sum())
    assert abs(lhs - float((g_color * d).sum())) <= 1e-12 * np.abs(g_color).sum()
    assert not g_pos[..., 2].any()                                                        # depth decides, it does not blend


def test_row_sums_of_a_rectangle_are_exact():
    """An axis-aligned rectangle of two triangles on a background: on rows away from its corners the antialiased mask sums to the
    rectangle's width in pixels, exactly (every t is a multiple of 1 / 256), its diagonal does not blend, and the sum's gradient in
    the x of the two right-hand vertices is 0.5 W / w per row."""
    h, w_img, w = 12, 16, 2.0
    x_lo, x_hi, y_lo, y_hi = 2 * 256 + 37, 12 * 256 + 201, 1 * 256 + 90, 10 * 256 + 150
    pos, tri = scenes.rectangle(x_lo, x_hi, y_lo, y_hi, w, h, w_img)
    out = ref.rasterize(pos, tri, h, w_img)
    ids, depth = out["tri"], out["depth"]
    topo = gref.edge_topology(tri)
    assert topo[0, 1] == 3 and topo[1, 2] == 1                      # the diagonal: a regular interior edge
    hits = gref.antialias_hits(pos, tri, topo, ids, depth, h, w_img)
    assert hits and not any((k["face"], k["edge"]) in ((0, 1), (1, 2)) for k in hits)
    mask = (ids >= 0).astype(np.float64)[..., None]
    assert len(np.unique(ids[0, 3:9])) == 3                         # both triangles and the background meet on these rows
    for dtype in (np.float64, np.float32):
        aa = gref.antialias(mask, hits, pos, h, w_img, dtype)
        rows = aa[0, 3:9, :, 0].astype(np.float64).sum(1)
        assert np.array_equal(rows, np.full(6, (x_hi - x_lo) / 256)), rows
        assert 0 < aa[0, 5, 2, 0] < 1 or 0 < aa[0, 5, 1, 0] < 1     # the left outline is blended
    cols = gref.antialias(mask, hits, pos, h, w_img, np.float64)[0, :, 4:11, 0].sum(0)
    assert np.array_equal(cols, np.full(7, (y_hi - y_lo) / 256))
    g = np.zeros((1, h, w_img, 1))
    g[0, 3:9] = 1
    _, g_pos = gref.antialias_grad(mask, hits, pos, g, h, w_img, np.float64)
    assert abs(g_pos[0, [1, 2], 0].sum() - 6 * 0.5 * w_img / w) <= 1e-12 * 6 * 0.5 * w_img / w
    assert abs(g_pos[0, [0, 3], 0].sum() + 6 * 0.5 * w_img / w) <= 1e-12 * 6 * 0.5 * w_img / w
