"""The two blend kernels (csrc/render_forward.hip, csrc/render_backward.hip) against the CPU oracle on images that are no
multiple of the 16 x 16 tile — the scenes of tests/edge_tile_scenes.py, whose properties
tests/test_edge_tile_scenes_cpu.py pins with the oracle alone.

csrc/api.hip rounds the tile grid up, so the last tile column or row of such an image is only partly inside it, and both
kernels rest on a chain of small agreements there.  Forward: a pixel outside the image is `done` from the first trip, a
terminated pixel stores no checkpoint, a wave whose 8 x 4 block lies outside is __all(done) at once, the final stores are
guarded by `inside`, and the image planes of view v sit at v * 3 * HW + c * HW, which for odd H * W is aligned to 4 bytes
only.  Backward: an outside pixel gets lastc = 0 and adds exact zeros to all twenty accumulators of fold_two_entries, the
checkpoint row is read at q * 64 + lane (the forward's cpix layout) and only where n_contrib > first.  What these scenes reach
and the whole-tile sizes of the rest of the suite do not: a backward segment with b > 0 in a partial tile (a checkpoint
read), a launch set at a ragged size, an image with odd H * W, an image smaller than one 8 x 8 quadrant, a 1 x 1 tile.

Bars.  Images and integer buffers as in test_gpu_deep_lists.py (IMG_TOL except at proven knife-edge pixels, at most
KNIFE_PIXEL_FRAC of the image: 0 pixels at 9 x 5).  Gradients: that module's _compare, twice per tensor
(compare_gradients).  First as it is: MAX_TOL of the whole tensor's largest |gradient| on every row that is no knife-edge
subject.  A Gaussian whose tiles are all partial tiles has a small gradient against that maximum (the largest shs gradient
among such rows is 5 % of the tensor maximum on "wide" and 0.7 % on "one_pixel"), so that bar alone lets those rows be
several per cent wrong.  Hence second, on edge_tile_scenes.edge_rows alone: MAX_TOL of the largest |gradient| among those
rows, and REL_TOL element by element above FLOOR_FRAC of it on the rows that share no knife-edge pixel, on at least
MIN_EDGE_ENTRIES entries (MAX_TOL, REL_TOL, FLOOR_FRAC and the knife-edge margin are that module's and the headline test's,
used through _compare).  The asserted figures use the oracle's backward given the alpha image of the HIP forward; the
oracle's own end-to-end backward is held to MAX_TOL where no pixel of the oracle's image is within a factor of two of the
0.9999 alpha cap (alpha < ALPHA_CAP: "cut_both" at azimuth 0, "sub_quadrant") and recorded otherwise.

The achieved figures are printed (pytest -s) and written as parity_edge_tiles.json next to the headline test's record
(test_gpu_headline_parity._dump) when that directory exists; profiles/parity_edge_tiles.json is a copy."""
import numpy as np
import pytest
import torch

import edge_tile_scenes as ets
from test_gpu_bucket_binning import _assert_equal, _render, plans  # noqa: F401  (plans: fixture)
from test_gpu_deep_lists import GRADS, KNIFE_PIXEL_FRAC, _compare, _hip_backward, _oracle_view, _upstream
from test_gpu_deep_lists import oracle8  # noqa: F401  (fixture)
from test_gpu_headline_parity import list_mode  # noqa: F401  (fixture)
from test_gpu_headline_parity import _dump as _write_record
from test_gpu_raster_parity import _assert_images, _check_forward_scene, _dev, _settings

pytestmark = pytest.mark.gpu

MIN_EDGE_ENTRIES = 100          # what the per-element bar has to cover among the edge rows of each tensor
ALPHA_CAP = 0.9998              # T_final = 1 - alpha below 2e-4: the walk ended, or nearly ended, at T (1 - alpha) < 1e-4
UPSTREAM_SEED = 17
FILLED = [n for n in ets.SCENES if n != "empty_edges"]
_report = {}


def _dump():
    _write_record(_report, "parity_edge_tiles.json")


def _tag(name, mode, extra=""):
    return name + extra + ("" if mode == "culled" else " / exact lists")


def _view(oracle, name, azimuth=0.0):
    """test_gpu_deep_lists._oracle_view of the scene plus its edge rows and whether the end-to-end figure is asserted."""
    o = _oracle_view(oracle, name, azimuth, mod=ets)
    if "edge" not in o:
        H, W = o["images"][0].shape[1:]
        o.update(edge=ets.edge_rows(o["ro"], H, W), below_cap=bool(float(o["images"][3].max()) < ALPHA_CAP))
    return o


def compare_gradients(tag, name, ours, ref, subjects, sharing, edge, cap, report, ref_end_to_end=None, assert_end_to_end=False):
    """test_gpu_deep_lists._compare on the whole tensor as it is, then on the `edge` rows alone: there the largest |ref| among
    those rows is the scale of MAX_TOL and of the floor of the per-element bar."""
    ours = ours.reshape(ref.shape)
    _compare(tag, name, ours, ref, subjects, cap, ref_end_to_end=ref_end_to_end, assert_end_to_end=assert_end_to_end, apart=sharing,
             report=report)
    _compare(tag, name + " / edge rows", ours[edge], ref[edge], subjects[edge], cap,
             ref_end_to_end=None if ref_end_to_end is None else ref_end_to_end[edge], assert_end_to_end=assert_end_to_end,
             sharing=sharing[edge], min_entries=MIN_EDGE_ENTRIES, report=report)


def _partial_pixels(H, W):
    """bool [H, W]: the pixels of the partial tiles."""
    return np.repeat(np.repeat(ets.partial_tiles(H, W), 16, 0), 16, 1)[:H, :W]


def _describe(tag, o, view=None):
    rec = dict(oracle_partial_tile_lists=o["lists"], knife_edge_pixels=o["knife_edge_pixels"], knife_edge_subject_rows=int(o["subjects"].sum()),
               rows_sharing_a_knife_edge_pixel=int(o["sharing"].sum()), edge_rows=int(o["edge"].sum()),
               edge_rows_sharing_a_knife_edge_pixel=int((o["sharing"] & o["edge"]).sum()), end_to_end_asserted=o["below_cap"])
    print(tag, rec)
    if view is None:
        _report.setdefault(tag, {}).update(rec)
    else:
        _report.setdefault(tag, {})["view %d" % view] = rec


@pytest.mark.parametrize("list_mode", ["culled", "exact"], indirect=True)
@pytest.mark.parametrize("name", list(ets.SCENES))
def test_forward_on_partial_tiles(oracle8, name, list_mode):
    """Records bit-exact, the kept lists the oracle's in its order, dropped entries proven dead, n_contrib equal; images
    within IMG_TOL except at proven knife-edge pixels, at most KNIFE_PIXEL_FRAC of the image."""
    from gaussianip_amd import rasterizer as R
    sc, cam, H, W = ets.build(name)
    stats, outs = {}, {}
    Rn, ro = _check_forward_scene(oracle8, sc, cam, H, W, ets.SH_DEGREE, ets.BG, nc_mismatch_frac=KNIFE_PIXEL_FRAC, min_keep=0.0,
                                  stats=stats, outputs=outs)
    keys, vals, ranges, tt, nc = ro.binning()
    length = ranges[:, 1].astype(np.int64) - ranges[:, 0].astype(np.int64)
    stats.update(oracle_num_rendered=Rn, oracle_segments=int(((length + 63) // 64).sum()))
    print(_tag(name, list_mode), "forward:", stats)
    _report.setdefault(_tag(name, list_mode), {})["forward"] = stats
    _dump()
    if list_mode == "exact":
        assert stats["num_rendered"] == Rn and stats["num_segments"] == stats["oracle_segments"], stats
    if name == "empty_edges":
        part = _partial_pixels(H, W)
        color, depth, alpha = (outs[k][0].cpu().numpy() for k in ("color", "depth", "alpha"))
        n_contrib = R.state_views(outs["plan"])["n_contrib"][0].cpu().numpy().reshape(H, W)
        assert int(length[ets.partial_tiles(H, W).reshape(-1)].max()) == 0
        for c in range(3):
            assert np.array_equal(color[c][part].view(np.uint32), np.full(int(part.sum()), ets.BG[c], np.float32).view(np.uint32)), c
        assert np.array_equal(alpha[0][part].view(np.uint32), np.zeros(int(part.sum()), np.uint32)), "alpha"
        assert np.array_equal(depth[0][part].view(np.uint32), np.zeros(int(part.sum()), np.uint32)), "depth"
        assert not n_contrib[part].any() and n_contrib[~part].any()


@pytest.mark.parametrize("list_mode", ["culled", "exact"], indirect=True)
@pytest.mark.parametrize("name", FILLED)
def test_backward_on_partial_tiles(oracle8, name, list_mode):
    """All six gradient tensors, all three upstream gradients given, against the oracle's backward: whole tensor and edge rows."""
    o = _view(oracle8, name)
    ro, (H, W) = o["ro"], o["images"][0].shape[1:]
    up = _upstream(UPSTREAM_SEED, 1, H, W)
    (color, radii, depth, alpha), g = _hip_backward(name, [0.0], up, mod=ets)
    assert np.array_equal(radii[0], o["images"][1]), "radii"
    go = ro.backward(up[0][0], up[1][0], up[2][0], alpha_out=alpha[0])
    go_e2e = ro.backward(up[0][0], up[1][0], up[2][0])
    tag = _tag(name, list_mode)
    _describe(tag, o)
    try:
        for k in GRADS:
            compare_gradients(tag, k, g[k][0] if k == "means2D" else g[k], go[k], o["subjects"], o["sharing"], o["edge"],
                              int(KNIFE_PIXEL_FRAC * H * W), _report, ref_end_to_end=go_e2e[k], assert_end_to_end=o["below_cap"])
    finally:
        _dump()


@pytest.mark.parametrize("list_mode", ["culled", "exact"], indirect=True)
def test_backward_with_empty_partial_tiles(oracle8, list_mode):
    """"empty_edges": every partial tile's list is empty.  Finite gradients, the oracle's within MAX_TOL, exact zeros on the
    rows of the culled Gaussians."""
    o = _view(oracle8, "empty_edges")
    ro, (H, W) = o["ro"], o["images"][0].shape[1:]
    up = _upstream(UPSTREAM_SEED, 1, H, W)
    (color, radii, depth, alpha), g = _hip_backward("empty_edges", [0.0], up, mod=ets)
    assert np.array_equal(radii[0], o["images"][1]), "radii"
    culled = radii[0] == 0
    assert int(culled.sum()) == ets.N_CULLED and not o["edge"].any()
    go = ro.backward(up[0][0], up[1][0], up[2][0], alpha_out=alpha[0])
    tag = _tag("empty_edges", list_mode)
    try:
        for k in GRADS:
            ours = g[k][0] if k == "means2D" else g[k]
            assert np.isfinite(ours).all() and float(np.abs(ours).max()) > 0.0, k
            assert not ours[culled].any(), k
            _compare(tag, k, ours, go[k], o["subjects"], int(KNIFE_PIXEL_FRAC * H * W), report=_report)
    finally:
        _dump()


def test_backward_with_dL_dcolor_alone_on_partial_tiles(oracle8, monkeypatch):
    """The stage-3 RGB loss: autograd.grad on `color` alone, so dL_ddepth and dL_dalpha reach the kernels as NULL pointers."""
    from gaussianip_amd import rasterizer as rz
    o = _view(oracle8, "cut_both")
    ro, (H, W) = o["ro"], o["images"][0].shape[1:]
    up = _upstream(UPSTREAM_SEED + 1, 1, H, W)
    seen = []
    orig = rz._run_backward
    monkeypatch.setattr(rz, "_run_backward", lambda plan, outs, gc, gd, ga: (seen.append((gc is None, gd is None, ga is None)),
                                                                             orig(plan, outs, gc, gd, ga))[1])
    (color, radii, depth, alpha), g = _hip_backward("cut_both", [0.0], up, color_only=True, mod=ets)
    assert seen == [(False, True, True)], seen
    go = ro.backward(up[0][0], None, None, alpha_out=alpha[0])
    go_e2e = ro.backward(up[0][0], None, None)
    _describe("cut_both / dL_dcolor only", o)
    try:
        for k in GRADS:
            compare_gradients("cut_both / dL_dcolor only", k, g[k][0] if k == "means2D" else g[k], go[k], o["subjects"], o["sharing"],
                              o["edge"], int(KNIFE_PIXEL_FRAC * H * W), _report, ref_end_to_end=go_e2e[k],
                              assert_end_to_end=o["below_cap"])
    finally:
        _dump()


@pytest.mark.parametrize("list_mode", ["culled", "exact"], indirect=True)
@pytest.mark.parametrize("name", ["cut_both", "one_pixel"])
def test_two_view_launch_set_on_partial_tiles(oracle8, name, list_mode):
    """Two azimuths in one launch set (H * W of "cut_both" is odd: the planes of view 1 start 4-byte aligned).  Each view's
    images and means2D gradients against that view's oracle, the parameter gradients against the float64 sum of the two oracle
    backwards under twice the per-view cap, and every view of the set against the same view rendered alone: radii, depth and
    alpha bit for bit, colour to the bar of test_multiview_equals_single_views (the launch set contracts its SH colours on
    the matrix cores, a single view does not).  A store that spills past a row end or a view boundary shows at a
    neighbouring pixel or in the next view."""
    azimuths = list(ets.azimuths(name))
    views = [_view(oracle8, name, az) for az in azimuths]
    H, W = views[0]["images"][0].shape[1:]
    up = _upstream(UPSTREAM_SEED + 2, 2, H, W)
    (color, radii, depth, alpha), g = _hip_backward(name, azimuths, up, mod=ets)
    cap = int(KNIFE_PIXEL_FRAC * H * W)
    tag = _tag(name, list_mode, " / 2 views")
    gos, e2es = [], []
    try:
        for v, o in enumerate(views):
            o_color, o_radii, o_depth, o_alpha = o["images"]
            _describe(tag, o, view=v)
            assert np.array_equal(radii[v], o_radii), "radii of view %d" % v
            _assert_images(o["ro"], torch.from_numpy(color[v]), torch.from_numpy(depth[v]), torch.from_numpy(alpha[v]), o_color,
                           o_depth, o_alpha, max_frac=KNIFE_PIXEL_FRAC)
            gos.append(o["ro"].backward(up[0][v], up[1][v], up[2][v], alpha_out=alpha[v]))
            e2es.append(o["ro"].backward(up[0][v], up[1][v], up[2][v]))
            compare_gradients(tag, "means2D[%d]" % v, g["means2D"][v], gos[v]["means2D"], o["subjects"], o["sharing"], o["edge"], cap,
                              _report, ref_end_to_end=e2es[v]["means2D"], assert_end_to_end=o["below_cap"])
            alone = _hip_backward(name, [azimuths[v]], tuple(u[v:v + 1] for u in up), mod=ets)[0]
            assert np.array_equal(alone[1][0], radii[v]) and np.array_equal(alone[2][0].view(np.uint32), depth[v].view(np.uint32))
            assert np.array_equal(alone[3][0].view(np.uint32), alpha[v].view(np.uint32)), "alpha of view %d" % v
            assert float(np.abs(alone[0][0] - color[v]).max()) < 1e-5, "colour of view %d" % v
        subjects = views[0]["subjects"] | views[1]["subjects"]
        below_cap = views[0]["below_cap"] and views[1]["below_cap"]
        for k in ("means3D", "opacities", "shs", "scales", "rotations"):
            _compare(tag, k, g[k], sum(x[k].astype(np.float64) for x in gos), subjects, 2 * cap,
                     ref_end_to_end=sum(x[k].astype(np.float64) for x in e2es), assert_end_to_end=below_cap,
                     apart=views[0]["sharing"] | views[1]["sharing"], report=_report)
    finally:
        _dump()


@pytest.mark.parametrize("views,list_mode", [(1, "culled"), (2, "culled"), (2, "exact")], indirect=["list_mode"])
def test_bucket_layout_equals_dense_bit_for_bit_on_partial_tiles(plans, monkeypatch, views, list_mode):
    """"cut_both": images, the six gradients, keys, tile_start, inst_offset, n_contrib and header words of the two key layouts."""
    name = "cut_both"
    sts = []
    for az in ets.azimuths(name)[:views]:
        sc, cam, H, W = ets.build(name, az)
        sts.append(_settings(cam, H, W, ets.BG, ets.SH_DEGREE))
    dense = _render(sc, sts, H, W, plans, monkeypatch, "dense")
    bucket = _render(sc, sts, H, W, plans, monkeypatch, "bucket")
    _assert_equal(bucket, dense, "%s, %d views" % (name, views))
    assert int(dense["header"][1]) == 0                                            # no overflow


@pytest.mark.parametrize("name", ["cut_both", "sub_quadrant"])
def test_forward_only_render_is_bit_identical_on_partial_tiles(monkeypatch, name):
    """A render under torch.no_grad() (GipRasterConfig::forward_only: no checkpoints kept) returns the training forward's images."""
    from gaussianip_amd import rasterize_views
    from gaussianip_amd import rasterizer as rz
    sts = []
    for az in ets.azimuths(name):
        sc, cam, H, W = ets.build(name, az)
        sts.append(_settings(cam, H, W, ets.BG, ets.SH_DEGREE))
    t = {k: _dev(v) for k, v in sc.items()}

    def render(grad):
        tt = {k: v.clone().requires_grad_(grad) for k, v in t.items()}
        with (torch.enable_grad() if grad else torch.no_grad()):
            return rasterize_views(tt["means3D"], None, tt["opacities"], sts, shs=tt["shs"], scales=tt["scales"], rotations=tt["rotations"])
    seen = []
    orig = rz._run_forward
    monkeypatch.setattr(rz, "_run_forward", lambda plan, cap, fo=False: (seen.append(bool(fo)), orig(plan, cap, fo))[1])
    with_state = render(True)
    without = render(False)
    torch.cuda.synchronize()
    assert seen[0] is False and seen[-1] is True, seen
    for a, b in zip(with_state, without):
        assert torch.equal(a, b)
    assert float(with_state[3].detach().max()) > 0.5


@pytest.mark.parametrize("list_mode", ["culled", "exact"], indirect=True)
def test_partial_tiles_are_bitwise_reproducible(list_mode):
    H, W = ets.SCENES["cut_both"][1:3]
    up = _upstream(UPSTREAM_SEED + 3, 1, H, W)
    a_img, a = _hip_backward("cut_both", [0.0], up, mod=ets)
    b_img, b = _hip_backward("cut_both", [0.0], up, mod=ets)
    for x, y in zip(a_img, b_img):
        assert np.array_equal(x, y)
    for k in GRADS:
        assert np.array_equal(a[k], b[k]), k
        assert np.isfinite(a[k]).all() and float(np.abs(a[k]).max()) > 0.0, k
