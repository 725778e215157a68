"""The scenes of tests/deep_list_scenes.py keep the properties tests/test_gpu_deep_lists.py relies on — checked with the
CPU oracle alone, so that a change to tests/scenes.py (or to the builder) cannot silently turn the long-list / deep-walk
GPU tests into short-list tests.

Measured (8 oracle threads, KNIFE_EDGE = 2e-5):
  scene    lists min / median / max   segments  n_contrib median / max  alpha image             knife-edge pixels / subjects
  long     37265 / 52603 / 72821      13503     2108 / 9227             all 0.9999              85 / 87   (0.10 %)
  deep      5641 / 11091 / 17405       2850    10174 / 17405            median 0.82, max 0.93   87 / 89   (0.15 %)
  deeper    9415 / 15492 / 24289       4056    14404 / 24289            median 0.93, max 0.976  268 / 285 (0.71 %)
  manyseg  17162 / 30248 / 43219      29659     1846 / 4875             all 0.9999              382 / 364 (0.61 %)"""
import numpy as np
import pytest

import deep_list_scenes as dls

KNIFE_EDGE = 2e-5


@pytest.fixture(scope="module")
def measured(oracle):
    oracle.set_threads(8)
    try:
        out = {}
        for name in dls.SCENES:
            ro, (color, radii, depth, alpha) = dls.oracle_forward(oracle, name)
            subjects, n_pixels = ro.knife_edge_gaussians(KNIFE_EDGE)
            out[name] = dict(dls.list_statistics(ro), alpha=alpha, visible=int((radii > 0).sum()), subjects=int(subjects.sum()),
                             knife_edge_pixels=n_pixels)
    finally:
        oracle.set_threads(1)
    return out


@pytest.mark.parametrize("name", ["long", "manyseg"])
def test_long_scenes_have_lists_beyond_the_on_chip_sort(measured, name):
    assert measured[name]["lists_max"] > 16384, measured[name]["lists_max"]


def test_manyseg_needs_a_second_trip_of_the_backward_grid(measured):
    assert measured["manyseg"]["segments"] > 16384, measured["manyseg"]["segments"]


@pytest.mark.parametrize("name", ["deep", "deeper"])
def test_deep_scenes_walk_to_the_end_of_their_lists_and_stay_translucent(measured, name):
    m = measured[name]
    assert m["n_contrib_median"] > 4096, m["n_contrib_median"]
    assert m["depth_share_median"] > 0.8, m["depth_share_median"]
    assert float((m["alpha"] > 0.999).mean()) <= 0.01


@pytest.mark.parametrize("name", list(dls.SCENES))
def test_knife_edge_subjects_are_few(measured, name):
    m = measured[name]
    assert m["visible"] > 0 and m["subjects"] <= 0.01 * m["visible"], (m["subjects"], m["visible"], m["knife_edge_pixels"])
