"""No kernel of csrc/ssim.hip may spill registers to scratch memory: the compile line and the parsing of
tests/test_no_kernel_spills_cpu.py (the Makefile's flags of libgip_model.so: -ffp-contract=off), nothing allowed to spill."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussianip_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ALLOWED = {}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_ssim_kernels_do_not_spill(tmp_path):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", os.path.join(CSRC, "ssim.hip"),
           "-o", str(tmp_path / "o.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    name, found, bad = None, [], []
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m and name:
            found.append(name)
            if int(m.group(1)) and not any(k in name for k in ALLOWED):
                bad.append((name, int(m.group(1))))
    for kernel in ("ssim_forward_kernel", "ssim_backward_kernel", "ssim_finish_kernel"):
        assert any(kernel in n for n in found), "no kernel-resource-usage remark for %s: %s" % (kernel, r.stderr[-500:])
    assert not bad, "kernels spilling to scratch: %s" % bad
