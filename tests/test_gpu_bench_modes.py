"""bench.py on one GPU: a plain run measures the headline raster step and nothing else (every secondary object of the line
is null), --dump-outputs still writes the last timed step, and --full adds the secondary objects behind it."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECONDARY = ("forward_only", "trained_state", "config4", "exact_lists", "replicas_layout", "roofline", "roofline_valu",
             "cpu_baseline", "ahds", "ahds_steps_per_s", "ahds_ms_per_step")


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--repeats", "3"] + list(args), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_measures_the_headline_only(tmp_path):
    d = _bench("--dump-outputs", str(tmp_path / "out"))
    assert d["metric"] == "raster_fwd_bwd_mpix_per_s" and d["unit"] == "Mpix/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0
    assert len(d["window_ms_per_step"]) == 3 and d["ms_per_step"] == sorted(d["window_ms_per_step"])[1]
    assert d["config"]["full"] is False and d["config"]["num_rendered_per_view"] is None
    for k in SECONDARY:
        assert d[k] is None, k
    written = sorted(os.listdir(tmp_path / "out"))
    assert written == sorted(n + ".npy" for n in d["dump_outputs"]["arrays"]) and "color.npy" in written


def test_full_run_adds_the_secondary_objects():
    d = _bench("--full", "--no-ahds", "--no-cpu-baseline", "--no-trained", "--no-exact", "--no-config4", "--profile-iters", "1")
    assert d["metric"] == "raster_fwd_bwd_mpix_per_s" and d["value"] > 0
    assert d["config"]["full"] is True and d["config"]["num_rendered_per_view"] > 0
    assert d["forward_only"]["ms_per_step"] > 0 and d["roofline"]["avg_launch_ms"] > 0
    for k in ("trained_state", "config4", "exact_lists", "cpu_baseline", "ahds"):
        assert d[k] is None, k                          # each left out by its own switch
