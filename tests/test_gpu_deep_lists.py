"""The backward blend (csrc/render_backward.hip, summed by csrc/gather_backward.hip) against the CPU oracle on tile lists
of tens of thousands of entries and on pixels that walk thousands of entries deep — the scenes of
tests/deep_list_scenes.py, whose properties tests/test_deep_list_scenes_cpu.py pins with the oracle alone.

What these scenes reach and the short lists of test_gpu_raster_parity.py / the 100k headline (58 entries on average) do not:
  * segments that start thousands of entries into a list (T and the prefix sums from checkpoint b - 1 with b in the
    hundreds; the forward's "terminated pixels store no checkpoint" and the backward's "n_contrib > first" must agree);
  * the prefix form dL/dalpha_j = T_j kappa_j + (Sp_{j+1} + Kc) / (1 - alpha_j) after thousands of fp32 additions;
  * entries at or beyond the tile's deepest n_contrib, whose rows must reach the gather as exact zeros (95 % of each
    list of "long" and "manyseg");
  * gradient rows of lists the tile sort handled beyond its on-chip path (more than 16384 keys);
  * the persistent grid's second trip (more than 16384 segments: "manyseg" with exact lists) and the uneven XCD split;
  * a backward with dL_dcolor alone (NULL dL_ddepth / dL_dalpha: the stage-3 RGB loss);
  * seg_tile / ckpt_start indexing of a second view (vt >= T) on deep lists.

Both list modes run: the default lists drop every provably dead entry, which on these nearly transparent splats is more
than half of each list (the alpha >= 1/255 region is much smaller than the 3-sigma rectangle), so only
GIP_RASTER_EXACT_LISTS=1 walks the full lengths of the scene table; the assertions on the library's own header below say
which mode reaches what.

Bars.  Images: IMG_TOL except at pixels the oracle PROVES to be knife-edge (oracle.pixel_margins < 2e-5), at most
KNIFE_PIXEL_FRAC of the image.  Gradients, with the oracle's backward given the alpha image of the HIP forward
(test_gpu_raster_parity._check_backward says why): MAX_TOL of the tensor's largest |gradient| on every row except the
oracle's knife-edge SUBJECT rows.  With opacities near 1/255 the Gaussian's G at the alpha threshold is 0.1-0.5, so one
threshold test that expf and v_exp_f32 decide differently moves that Gaussian's opacity and geometry gradient by several
per cent of the tensor maximum (about 1e-3 at the usual opacities).  Subject rows are still compared: each one that
misses the bar needs at least one flipped pixel, so their number is bounded by the pixel cap.  On "deep" and "deeper"
also the headline test's per-element bar (REL_TOL above FLOOR_FRAC of the maximum) on every row that shares no pixel with
a knife-edge subject, and the end-to-end comparison (oracle backward on the oracle's own alpha image) at MAX_TOL; on
"long" and "manyseg" every pixel sits at the 0.9999 alpha cap, where T_final := 1 - alpha_out turns the two forwards'
rounding into per-cent differences, so the end-to-end figure is recorded only.
On those two scenes the isolated figure is not rounding either: it is the one knife-edge pixel of the forward test.  "long"
measures 1.7e-3 on means3D / opacities in both list modes, and the oracle alone reproduces that figure to two digits when
its alpha image is changed at pixel (30, 4) as if the walk had blended the one entry whose T (1 - alpha) < 1e-4 test sits
8e-7 from flipping (list position 2529, alpha 0.015): through T_final := 1 - alpha_out the flip scales every T_j of that
pixel by 1 - alpha, for every Gaussian blended there and not only for the subject.  The rows that share no pixel with a
knife-edge subject (94 % of the Gaussians) agree to 1.5e-5, and that figure is recorded next to the asserted one.
The achieved figures are printed (pytest -s) and written as parity_deep_lists.json next to the headline test's record
(test_gpu_headline_parity._dump) when that directory exists; profiles/parity_deep_lists.json is a copy."""

import numpy as np
import pytest
import torch

import deep_list_scenes as dls
from test_gpu_headline_parity import FLOOR_FRAC, REL_TOL, list_mode  # noqa: F401  (list_mode: fixture)
from test_gpu_headline_parity import _dump as _write_record
from test_gpu_raster_parity import KNIFE_EDGE, _assert_images, _check_forward_scene, _dev, _settings

pytestmark = pytest.mark.gpu

MAX_TOL = 2e-3
KNIFE_PIXEL_FRAC = 2e-3             # the cap the suite uses for its adversarial scenes: 8 pixels at 64 x 64, 32 at 144 x 112
MIN_ELEMENTWISE_ENTRIES = 1000
GRADS = ("means3D", "means2D", "opacities", "shs", "scales", "rotations")
_report = {}
_oracle_cache = {}


@pytest.fixture
def oracle8(oracle):
    oracle.set_threads(8)
    yield oracle
    oracle.set_threads(1)


def _dump():
    _write_record(_report, "parity_deep_lists.json")


def _oracle_view(oracle, name, azimuth=0.0, mod=dls):
    """The oracle's forward of one view, its images and its knife-edge classes: computed once per (scene, camera).  `mod`: the
    scenes module (deep_list_scenes, or one with its build / oracle_forward / list_statistics / BG / SH_DEGREE)."""
    key = (mod.__name__, name, azimuth)
    if key not in _oracle_cache:
        ro, images = mod.oracle_forward(oracle, name, azimuth)
        subjects, n_pixels, sharing = ro.knife_edge_gaussians(KNIFE_EDGE, sharing=True)
        _oracle_cache[key] = dict(ro=ro, images=images, subjects=subjects, sharing=sharing | subjects, knife_edge_pixels=n_pixels,
                                  lists=mod.list_statistics(ro))
    return _oracle_cache[key]


def _upstream(seed, V, H, W):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(V, 3, H, W)).astype(np.float32), rng.normal(size=(V, 1, H, W)).astype(np.float32),
            rng.normal(size=(V, 1, H, W)).astype(np.float32))


def _hip_backward(name, azimuths, up, color_only=False, mod=dls):
    """Forward + backward of the launch set through the autograd function.  Returns (images, {name: gradient}) as numpy;
    means2D is [V, P, 3]."""
    from gaussianip_amd import GaussianRasterizer, rasterize_views
    V = len(azimuths)
    sts = []
    for az in azimuths:
        sc, cam, H, W = mod.build(name, az)
        sts.append(_settings(cam, H, W, mod.BG, mod.SH_DEGREE))
    P = sc["means3D"].shape[0]
    t = {k: _dev(v).requires_grad_(True) for k, v in sc.items()}
    kw = dict(shs=t["shs"], scales=t["scales"], rotations=t["rotations"])
    if V == 1:          # the reference call
        m2 = torch.zeros(P, 3, device="cuda", requires_grad=True)
        outs = GaussianRasterizer(sts[0])(means3D=t["means3D"], means2D=m2, opacities=t["opacities"], **kw)
        color, radii, depth, alpha = (o[None] for o in outs)
    else:
        m2 = torch.zeros(V, P, 3, device="cuda", requires_grad=True)
        color, radii, depth, alpha = rasterize_views(t["means3D"], m2, t["opacities"], sts, **kw)
    leaves = [t["means3D"], m2, t["opacities"], t["shs"], t["scales"], t["rotations"]]
    gC, gD, gA = (_dev(u) for u in up)
    if color_only:
        g = torch.autograd.grad([color], leaves, [gC])
    else:
        g = torch.autograd.grad([color, depth, alpha], leaves, [gC, gD, gA])
    torch.cuda.synchronize()
    grads = {k: v.detach().cpu().numpy() for k, v in zip(GRADS, g)}
    grads["means2D"] = grads["means2D"].reshape(V, P, 3)
    return tuple(o.detach().cpu().numpy() for o in (color, radii, depth, alpha)), grads


def _library_lists(name):
    """What the library's own binning made of the scene in the current list mode (header words of a no-grad forward)."""
    from gaussianip_amd import rasterizer as R
    sc, cam, H, W = dls.build(name)
    _, plan = R.forward_with_state(_dev(sc["means3D"]), _dev(sc["opacities"]), [_settings(cam, H, W, dls.BG, dls.SH_DEGREE)],
                                   shs=_dev(sc["shs"]), scales=_dev(sc["scales"]), rotations=_dev(sc["rotations"]))
    torch.cuda.synchronize()
    hdr = R.state_views(plan)["header"].cpu().numpy()
    assert int(hdr[2]) == 0, "overflow"
    return dict(num_rendered=int(hdr[1]), max_tile_count=int(hdr[3]), num_segments=int(hdr[5]))


def _assert_reach(name, mode, lib):
    """The paths a scene is there for were really walked by the library (not only by the oracle's longer lists)."""
    if name in ("long", "manyseg"):
        assert lib["max_tile_count"] > 16384, lib        # tile sort beyond its on-chip path
    if name == "manyseg" and mode == "exact":
        assert lib["num_segments"] > 16384, lib          # second trip of the backward's persistent grid


def _row_errors(ours, ref, top):
    P = ref.shape[0]
    return (np.abs(ours.astype(np.float64).reshape(ref.shape) - ref) / top).reshape(P, -1).max(1)


def _compare(tag, name, ours, ref, subjects, cap, ref_end_to_end=None, assert_end_to_end=False, sharing=None, apart=None,
             min_entries=MIN_ELEMENTWISE_ENTRIES, report=None):
    """MAX_TOL of the largest |gradient| on every row that is no knife-edge subject; at most `cap` subject rows beyond it;
    `sharing` given: REL_TOL element by element above FLOOR_FRAC of the maximum on the rows outside `sharing`;
    `apart` given: the max-normalised error over the rows outside it is recorded as well.  `min_entries`: what the per-element
    bar has to cover at least; `report`: the record to write to (this module's by default)."""
    ref = ref.astype(np.float64)
    top = float(np.abs(ref).max()) + 1e-30
    rows = _row_errors(ours, ref, top)
    e_max = float(rows[~subjects].max())
    n_subject_miss = int((rows[subjects] >= MAX_TOL).sum())
    rec = dict(max_norm=e_max, top=top, subject_rows=int(subjects.sum()), subject_rows_beyond_bar=n_subject_miss,
               subject_rows_worst=float(rows[subjects].max()) if subjects.any() else 0.0)
    line = "%-28s %-11s max-normalised %.2e   subject rows beyond the bar %d of %d (worst %.2e)" % (
        tag, name, e_max, n_subject_miss, int(subjects.sum()), rec["subject_rows_worst"])
    e_rel = n_rel = None
    if sharing is not None:
        big = np.abs(ref) > FLOOR_FRAC * top
        big[sharing] = False
        n_rel = int(big.sum())
        e_rel = float((np.abs(ours.astype(np.float64).reshape(ref.shape) - ref)[big] / np.abs(ref[big])).max()) if n_rel else 0.0
        rec.update(rel=e_rel, entries_checked=n_rel)
        line += "   per-element relative %.2e on %d entries" % (e_rel, n_rel)
    if apart is not None:
        rec["max_norm_sharing_no_knife_edge_pixel"] = float(rows[~apart].max())
        line += "   rows sharing no knife-edge pixel %.2e" % rec["max_norm_sharing_no_knife_edge_pixel"]
    e2e = None
    if ref_end_to_end is not None:
        e2e = float(_row_errors(ours, ref_end_to_end.astype(np.float64), top)[~subjects].max())
        rec["max_norm_end_to_end"] = e2e
        line += "   end-to-end %.2e%s" % (e2e, "" if assert_end_to_end else " (recorded only)")
    (_report if report is None else report).setdefault(tag, {})[name] = rec
    print(line)
    assert e_max < MAX_TOL, "%s %s: max error / max |grad| = %.3e outside the knife-edge subject rows" % (tag, name, e_max)
    assert n_subject_miss <= cap, "%s %s: %d knife-edge subject rows miss the bar, more than the %d pixels that may flip" % (
        tag, name, n_subject_miss, cap)
    if sharing is not None:
        assert n_rel >= min_entries, "%s %s: the per-element bar covers only %d entries" % (tag, name, n_rel)
        assert e_rel < REL_TOL, "%s %s: per-element relative error %.3e (entries above %.0e of the maximum)" % (tag, name, e_rel, FLOOR_FRAC)
    if assert_end_to_end:
        assert e2e < MAX_TOL, "%s %s: end-to-end max error / max |grad| = %.3e" % (tag, name, e2e)


def _tag(name, mode, extra=""):
    return name + extra + ("" if mode == "culled" else " / exact lists")


@pytest.mark.parametrize("name,list_mode", [("long", "culled"), ("deep", "culled"), ("deeper", "culled"), ("manyseg", "culled"),
                                            ("long", "exact"), ("manyseg", "exact")], indirect=["list_mode"])
def test_forward_on_long_and_deep_lists(oracle8, name, list_mode):
    """Records bit-exact, the kept lists the oracle's in its order, dropped entries proven dead, n_contrib equal; images
    within IMG_TOL except at proven knife-edge pixels, at most KNIFE_PIXEL_FRAC of the image."""
    sc, cam, H, W = dls.build(name)
    stats = {}
    Rn, ro = _check_forward_scene(oracle8, sc, cam, H, W, dls.SH_DEGREE, dls.BG, nc_mismatch_frac=KNIFE_PIXEL_FRAC, min_keep=0.0,
                                  stats=stats)
    stats.update(oracle_num_rendered=Rn, oracle_lists=dls.list_statistics(ro))
    print(_tag(name, list_mode), "forward:", stats)
    _report.setdefault(_tag(name, list_mode), {})["forward"] = stats
    _dump()
    # what the library itself walked: the tile sort's beyond-LDS path in either mode, and with exact lists the oracle's lengths
    _assert_reach(name, list_mode, stats)
    if name in ("deep", "deeper"):
        assert stats["n_contrib_median"] > 4096 and stats["n_contrib_median"] > 0.8 * stats["lists_median"], stats
    if list_mode == "exact":
        assert stats["num_rendered"] == Rn and stats["num_segments"] == stats["oracle_lists"]["segments"], stats


@pytest.mark.parametrize("list_mode", ["culled", "exact"], indirect=True)
@pytest.mark.parametrize("name", ["long", "deep", "deeper", "manyseg"])
def test_backward_on_long_and_deep_lists(oracle8, name, list_mode):
    """All six gradient tensors, all three upstream gradients given, against the oracle's backward."""
    o = _oracle_view(oracle8, name)
    ro, (H, W) = o["ro"], o["images"][0].shape[1:]
    up = _upstream(17, 1, H, W)
    (color, radii, depth, alpha), g = _hip_backward(name, [0.0], up)
    assert np.array_equal(radii[0], o["images"][1]), "radii"
    go = ro.backward(up[0][0], up[1][0], up[2][0], alpha_out=alpha[0])
    go_e2e = ro.backward(up[0][0], up[1][0], up[2][0])
    deep = name in ("deep", "deeper")
    cap = int(KNIFE_PIXEL_FRAC * H * W)
    tag = _tag(name, list_mode)
    print("%s: oracle lists %s, %d knife-edge pixels, %d subject rows, %d rows share a knife-edge pixel" % (
        tag, o["lists"], o["knife_edge_pixels"], int(o["subjects"].sum()), int(o["sharing"].sum())))
    lib = _library_lists(name)
    _assert_reach(name, list_mode, lib)
    _report.setdefault(tag, {}).update(oracle_lists=o["lists"], library_lists=lib, knife_edge_pixels=o["knife_edge_pixels"],
                                       rows_sharing_a_knife_edge_pixel=int(o["sharing"].sum()))
    try:
        for k in GRADS:
            _compare(tag, k, g[k][0] if k == "means2D" else g[k], go[k], o["subjects"], cap, ref_end_to_end=go_e2e[k],
                     assert_end_to_end=deep, sharing=o["sharing"] if deep else None, apart=None if deep else o["sharing"])
    finally:
        _dump()


def test_backward_with_dL_dcolor_alone_on_deep_lists(oracle8, monkeypatch):
    """The stage-3 RGB loss: autograd.grad on `color` alone, so dL_ddepth and dL_dalpha reach the kernels as NULL pointers."""
    from gaussianip_amd import rasterizer as rz
    o = _oracle_view(oracle8, "deep")
    ro, (H, W) = o["ro"], o["images"][0].shape[1:]
    up = _upstream(18, 1, H, W)
    seen = []
    orig = rz._run_backward
    monkeypatch.setattr(rz, "_run_backward", lambda plan, outs, gc, gd, ga: (seen.append((gc is None, gd is None, ga is None)),
                                                                             orig(plan, outs, gc, gd, ga))[1])
    (color, radii, depth, alpha), g = _hip_backward("deep", [0.0], up, color_only=True)
    assert seen == [(False, True, True)], seen
    go = ro.backward(up[0][0], None, None, alpha_out=alpha[0])
    go_e2e = ro.backward(up[0][0], None, None)
    try:
        for k in GRADS:
            _compare("deep / dL_dcolor only", k, g[k][0] if k == "means2D" else g[k], go[k], o["subjects"], int(KNIFE_PIXEL_FRAC * H * W),
                     ref_end_to_end=go_e2e[k], assert_end_to_end=True, sharing=o["sharing"])
    finally:
        _dump()


@pytest.mark.parametrize("list_mode", ["culled", "exact"], indirect=True)
def test_two_view_launch_set_on_deep_lists(oracle8, list_mode):
    """"deep" from azimuth 0 and 90 in one launch set: each view's images and means2D gradients against that view's oracle,
    the parameter gradients against the float64 sum of the two oracle backwards.  A row of the sum may miss the bar if it
    is a knife-edge subject in either view, so the cap on such rows is the sum of the two views' pixel caps."""
    azimuths = [0.0, 90.0]
    views = [_oracle_view(oracle8, "deep", az) for az in azimuths]
    H, W = views[0]["images"][0].shape[1:]
    up = _upstream(19, 2, H, W)
    (color, radii, depth, alpha), g = _hip_backward("deep", azimuths, up)
    cap = int(KNIFE_PIXEL_FRAC * H * W)
    tag = _tag("deep", list_mode, " / 2 views")
    gos, e2es = [], []
    try:
        for v, o in enumerate(views):
            o_color, o_radii, o_depth, o_alpha = o["images"]
            assert np.array_equal(radii[v], o_radii), "radii of view %d" % v
            _assert_images(o["ro"], torch.from_numpy(color[v]), torch.from_numpy(depth[v]), torch.from_numpy(alpha[v]), o_color,
                           o_depth, o_alpha, max_frac=KNIFE_PIXEL_FRAC)
            gos.append(o["ro"].backward(up[0][v], up[1][v], up[2][v], alpha_out=alpha[v]))
            e2es.append(o["ro"].backward(up[0][v], up[1][v], up[2][v]))
            _compare(tag, "means2D[%d]" % v, g["means2D"][v], gos[v]["means2D"], o["subjects"], cap, ref_end_to_end=e2es[v]["means2D"],
                     assert_end_to_end=True, sharing=o["sharing"])
        subjects = views[0]["subjects"] | views[1]["subjects"]
        sharing = views[0]["sharing"] | views[1]["sharing"]
        for k in ("means3D", "opacities", "shs", "scales", "rotations"):
            _compare(tag, k, g[k], sum(x[k].astype(np.float64) for x in gos), subjects, 2 * cap,
                     ref_end_to_end=sum(x[k].astype(np.float64) for x in e2es), assert_end_to_end=True, sharing=sharing)
    finally:
        _dump()


@pytest.mark.parametrize("list_mode", ["culled", "exact"], indirect=True)
def test_backward_over_many_segments_is_bitwise_reproducible(list_mode):
    """"manyseg" twice: with exact lists more than 16384 segments, i.e. the persistent grid's second trip."""
    H, W = dls.SCENES["manyseg"][1:3]
    _assert_reach("manyseg", list_mode, _library_lists("manyseg"))
    up = _upstream(20, 1, H, W)
    a_img, a = _hip_backward("manyseg", [0.0], up)
    b_img, b = _hip_backward("manyseg", [0.0], up)
    for x, y in zip(a_img, b_img):
        assert np.array_equal(x, y)
    for k in GRADS:
        assert np.array_equal(a[k], b[k]), k
        assert np.isfinite(a[k]).all() and float(np.abs(a[k]).max()) > 0.0, k
