"""The scenes of tests/edge_tile_scenes.py keep the properties tests/test_gpu_edge_tiles.py relies on — checked with the CPU
oracle alone, for every camera the GPU tests use: the partial tiles are filled more than two 64-entry segments deep, enough
Gaussians live in partial tiles alone, knife-edge pixels stay within the suite's cap (not raised for small images: 0 pixels
at 9 x 5) and the per-element bar of the edge rows covers at least MIN_EDGE_ENTRIES entries of every tensor.

Then a test of the test: the oracle's own gradients of "wide" with the edge rows of `shs` multiplied by 1.02.  The largest
shs gradient among those rows is 5 % of the tensor maximum, so the bar of test_gpu_raster_parity._check_backward over the
whole tensor accepts the change (1e-3 < 2e-3); test_gpu_edge_tiles.compare_gradients has to reject it.

Measured (KNIFE_EDGE = 2e-5; lists and deepest n_contrib of the partial tiles that are to be filled; the last two columns
are the fewest entries of a tensor above the floor of the edge rows' per-element bar, always `opacities`, and the smallest
share a tensor's largest edge-row gradient has of the tensor's maximum):
  scene         camera  entries    deepest n_contrib  edge rows  knife-edge pixels / cap  entries  smallest share
  cut_both        0     279-687    278-687            328        0 / 2                    241      0.45  (shs)
  cut_both       90     275-662    275-662            354        1 / 2                    258      0.14  (shs)
  one_pixel       0     232-357    232-357            328        1 / 1                    290      0.007 (shs)
  one_pixel     120     237-337    237-331            327        0 / 1                    286      0.005 (shs)
  sub_quadrant    0     583        583                583        0 / 0                    502      1
  half_tile       0     190-660    188-660            166        1 / 1                    139      0.047 (opacities)
  wide            0     140-433    140-433            257        0 / 7                    169      0.052 (shs)"""
import numpy as np
import pytest

import edge_tile_scenes as ets
from test_gpu_deep_lists import GRADS, KNIFE_PIXEL_FRAC, _upstream
from test_gpu_edge_tiles import FILLED, MIN_EDGE_ENTRIES, UPSTREAM_SEED, compare_gradients
from test_gpu_headline_parity import FLOOR_FRAC
from test_gpu_raster_parity import BACKWARD_TOL, KNIFE_EDGE, _max_norm_error

MIN_LIST = 130              # more than two 64-entry segments
MIN_DEPTH = 128
MIN_EDGE_ROWS = 100
CAMERAS = [(name, az) for name in ets.SCENES for az in ets.azimuths(name)]


@pytest.fixture(scope="module")
def measured(oracle):
    oracle.set_threads(8)
    try:
        out = {}
        for name, az in CAMERAS:
            ro, (color, radii, depth, alpha) = ets.oracle_forward(oracle, name, az)
            H, W = alpha.shape[1:]
            subjects, n_pixels, sharing = ro.knife_edge_gaussians(KNIFE_EDGE, sharing=True)
            up = _upstream(UPSTREAM_SEED, 1, H, W)
            out[name, az] = dict(ro=ro, H=H, W=W, radii=radii, lists=ets.list_statistics(ro), edge=ets.edge_rows(ro, H, W), subjects=subjects,
                                 sharing=sharing | subjects, knife_edge_pixels=n_pixels, grads=ro.backward(up[0][0], up[1][0], up[2][0]))
    finally:
        oracle.set_threads(1)
    return out


def test_the_table_names_the_sizes_it_is_there_for():
    sizes = {name: ets.SCENES[name][1:3] for name in ets.SCENES}
    assert sizes == dict(cut_both=(41, 27), one_pixel=(17, 33), sub_quadrant=(9, 5), half_tile=(24, 40), wide=(50, 75), empty_edges=(41, 27))
    assert sorted(CAMERAS) == sorted([(n, 0.0) for n in ets.SCENES] + [("cut_both", 90.0), ("one_pixel", 120.0)])


@pytest.mark.parametrize("name,az", CAMERAS)
def test_partial_tiles_are_filled_two_segments_deep(measured, name, az):
    m = measured[name, az]
    assert len(m["lists"]) == int(ets.partial_tiles(m["H"], m["W"]).sum()) > 0
    for tile, st in m["lists"].items():
        if name == "empty_edges":
            assert st["entries"] == 0 and st["n_contrib_max"] == 0, (tile, st)
        elif not (name == "one_pixel" and st["pixels"] == 1):
            assert st["entries"] >= MIN_LIST and st["n_contrib_max"] > MIN_DEPTH, (tile, st)
    if name == "empty_edges":
        assert int((m["radii"] == 0).sum()) == ets.N_CULLED and int((m["radii"] > 0).sum()) == ets.SCENES[name][0] - ets.N_CULLED
    if name == "one_pixel":
        assert sorted(st["pixels"] for st in m["lists"].values()) == [1, 16, 16, 16]


@pytest.mark.parametrize("name,az", [c for c in CAMERAS if c[0] != "empty_edges"])
def test_enough_gaussians_live_in_partial_tiles_alone(measured, name, az):
    m = measured[name, az]
    assert int(m["edge"].sum()) >= MIN_EDGE_ROWS, int(m["edge"].sum())
    assert not (m["edge"] & (m["radii"] == 0)).any()


def test_edge_rows_are_the_gaussians_without_an_instance_in_a_full_tile(measured):
    """edge_rows against a plain loop over the oracle's lists."""
    m = measured["wide", 0.0]
    keys, vals, ranges, tt, nc = m["ro"].binning()
    part = ets.partial_tiles(m["H"], m["W"]).reshape(-1)
    in_full, in_partial = set(), set()
    for t in range(ranges.shape[0]):
        (in_partial if part[t] else in_full).update(vals[int(ranges[t, 0]):int(ranges[t, 1])].tolist())
    assert set(np.flatnonzero(m["edge"]).tolist()) == in_partial - in_full
    assert part.reshape(4, 5).tolist() == [[False] * 4 + [True]] * 3 + [[True] * 5]


@pytest.mark.parametrize("name,az", CAMERAS)
def test_knife_edge_pixels_stay_within_the_cap(measured, name, az):
    m = measured[name, az]
    assert m["knife_edge_pixels"] <= int(KNIFE_PIXEL_FRAC * m["H"] * m["W"]), m["knife_edge_pixels"]


def _entries_above_the_floor(m, k):
    ref = np.abs(m["grads"][k].astype(np.float64))[m["edge"] & ~m["sharing"]]
    top_edge = float(np.abs(m["grads"][k][m["edge"]]).max())
    return int((ref > FLOOR_FRAC * top_edge).sum())


@pytest.mark.parametrize("name,az", [c for c in CAMERAS if c[0] != "empty_edges"])
def test_the_per_element_bar_of_the_edge_rows_covers_every_tensor(measured, name, az):
    m = measured[name, az]
    counts = {k: _entries_above_the_floor(m, k) for k in GRADS}
    print(name, az, counts)
    assert min(counts.values()) >= MIN_EDGE_ENTRIES, counts


def test_the_whole_tensor_bar_accepts_edge_rows_two_per_cent_off_and_the_edge_row_bar_does_not(measured):
    m = measured["wide", 0.0]
    ref = m["grads"]["shs"]
    off = ref.copy()
    off[m["edge"]] *= np.float32(1.02)
    share = float(np.abs(ref[m["edge"]]).max() / np.abs(ref).max())
    assert 0.01 < share < 0.09, share
    assert _max_norm_error(off, ref) < BACKWARD_TOL                   # what every backward test of the suite asserts
    cap = int(KNIFE_PIXEL_FRAC * m["H"] * m["W"])
    args = ("wide / oracle against itself", "shs")
    compare_gradients(*args, ref, ref, m["subjects"], m["sharing"], m["edge"], cap, {})
    with pytest.raises(AssertionError, match="shs / edge rows"):
        compare_gradients(*args, off, ref, m["subjects"], m["sharing"], m["edge"], cap, {})


def test_filled_scenes_are_all_but_empty_edges():
    assert FILLED == ["cut_both", "one_pixel", "sub_quadrant", "half_tile", "wide"]
