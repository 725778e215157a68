"""Bucket mode of the tile binning, the parts that need no GPU: the stride rule, the host policy that chooses between the
bucketed and the dense key layout, and the register budget of the preprocess kernel that now stores the keys itself.

The policy (gaussianip_amd/rasterizer.py): bucket mode needs a longest-list hint for the shape, V * T * S * 8 bytes within the
budget, and GIP_RASTER_BUCKETS != 0; otherwise the call is dense."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussianip_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KEY = (0, 1000, 4, 1024, 1024, False)         # device, P, V, H, W of the capacity hint + the list mode (rasterizer._bucket_key)


@pytest.fixture
def policy(monkeypatch):
    from gaussianip_amd import rasterizer as R
    monkeypatch.setattr(R, "_bucket_hint", {})
    monkeypatch.delenv("GIP_RASTER_BUCKETS", raising=False)
    monkeypatch.delenv("GIP_RASTER_BUCKET_BYTES", raising=False)
    return R


@pytest.mark.parametrize("last_max", [0, 1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 511, 512, 513, 2047, 2048, 2803, 16384, 100000])
def test_stride_is_the_smallest_odd_multiple_of_32_above_the_bound(policy, last_max):
    S = policy.bucket_stride(last_max)
    bound = 2 * last_max + 64
    assert S % 32 == 0 and (S // 32) % 2 == 1, S            # bytes: an odd multiple of 256
    assert S >= bound
    smaller = [m * 32 for m in range(1, S // 32, 2) if m * 32 >= bound]
    assert not smaller, (S, smaller)


def test_first_call_of_a_shape_is_dense(policy, monkeypatch):
    assert policy._pick_stride(KEY, 4, 1024, 1024) == 0
    policy._bucket_hint[KEY] = 2803
    assert policy._pick_stride(KEY, 4, 1024, 1024) == policy.bucket_stride(2803) == 5728
    assert policy._pick_stride((0, 1001, 4, 1024, 1024, False), 4, 1024, 1024) == 0       # another P: another shape
    assert policy._pick_stride(KEY[:5] + (True,), 4, 1024, 1024) == 0                     # exact lists: longer lists, their own hint
    monkeypatch.setenv("GIP_RASTER_EXACT_LISTS", "1")
    assert policy._bucket_key(KEY[:5]) == KEY[:5] + (True,)
    monkeypatch.setenv("GIP_RASTER_EXACT_LISTS", "0")
    assert policy._bucket_key(KEY[:5]) == KEY


def test_env_switch_forces_the_dense_layout(policy, monkeypatch):
    policy._bucket_hint[KEY] = 100
    assert policy._pick_stride(KEY, 4, 1024, 1024) > 0
    monkeypatch.setenv("GIP_RASTER_BUCKETS", "0")
    assert policy._pick_stride(KEY, 4, 1024, 1024) == 0
    monkeypatch.setenv("GIP_RASTER_BUCKETS", "1")
    assert policy._pick_stride(KEY, 4, 1024, 1024) > 0


def test_budget_fallback(policy, monkeypatch):
    policy._bucket_hint[KEY] = 2803
    S, tiles = 5728, 4 * 64 * 64
    assert policy._bucket_budget() == 2 << 30 and tiles * S * 8 <= 2 << 30
    monkeypatch.setenv("GIP_RASTER_BUCKET_BYTES", str(tiles * S * 8))
    assert policy._pick_stride(KEY, 4, 1024, 1024) == S                            # exactly the budget: bucket mode
    monkeypatch.setenv("GIP_RASTER_BUCKET_BYTES", str(tiles * S * 8 - 1))
    assert policy._pick_stride(KEY, 4, 1024, 1024) == 0
    monkeypatch.delenv("GIP_RASTER_BUCKET_BYTES")
    policy._bucket_hint[KEY] = 20000                                               # 16384 tiles x 40096 entries x 8 B > 2 GiB
    assert policy._pick_stride(KEY, 4, 1024, 1024) == 0
    # a partly covered last tile row / column counts as a tile
    policy._bucket_hint[(0, 10, 1, 17, 33, False)] = 0
    monkeypatch.setenv("GIP_RASTER_BUCKET_BYTES", str(2 * 3 * 96 * 8 - 1))
    assert policy._pick_stride((0, 10, 1, 17, 33, False), 1, 17, 33) == 0
    monkeypatch.setenv("GIP_RASTER_BUCKET_BYTES", str(2 * 3 * 96 * 8))
    assert policy._pick_stride((0, 10, 1, 17, 33, False), 1, 17, 33) == 96


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_preprocess_keeps_two_workgroups_per_cu(tmp_path):
    """The kernel that now stores the keys runs 1024-thread workgroups, two per CU: at most 64 VGPRs and no scratch
    (DESIGN.md §4 records what 90 registers cost).  Compiled with the Makefile's flags for this source."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    common = re.search(r"^COMMON = (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").replace("-I../../include", "-I" + os.path.join(ROOT, "include"))
    exact = re.search(r"^EXACT = (.*)$", mk, re.M).group(1)
    assert "preprocess" in re.search(r"^SRCS_EXACT = (.*)$", mk, re.M).group(1).split()
    cmd = [HIPCC] + common.split() + exact.split() + ["-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c",
                                                      os.path.join(CSRC, "preprocess.hip"), "-o", str(tmp_path / "o.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"remark:\s+(VGPRs|ScratchSize \[bytes/lane\]|AGPRs): (\d+)", ln)
        if m and name:
            usage.setdefault(name, {})[m.group(1).split()[0]] = int(m.group(2))
    pre = [v for k, v in usage.items() if "gip_preprocess_kernel" in k]
    assert len(pre) == 1, sorted(usage)
    print("gip_preprocess_kernel:", pre[0])
    assert pre[0]["VGPRs"] <= 64 and pre[0].get("AGPRs", 0) == 0 and pre[0]["ScratchSize"] == 0, pre[0]
