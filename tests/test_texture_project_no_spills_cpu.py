"""No kernel of csrc/texture_project.hip may spill registers to scratch memory: the compile line and the parsing of
tests/test_texture_no_spills_cpu.py (the Makefile's flags of libgip_model.so: -ffp-contract=off), nothing allowed to spill.  The
kernel keeps a texel's point, normal and four sums per lane and loops over the views without a local array."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussianip_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("texture_project_kernel",)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_texture_project_kernels_do_not_spill(tmp_path):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", os.path.join(CSRC, "texture_project.hip"),
           "-o", str(tmp_path / "o.o")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    name, scratch, spilled = None, {}, {}
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m and name:
            scratch[name] = int(m.group(1))
        m = re.search(r"[SV]GPRs Spill: (\d+)", ln)
        if m and name:
            spilled[name] = spilled.get(name, 0) + int(m.group(1))
    for kernel in KERNELS:
        assert any(kernel in n for n in scratch), "no kernel-resource-usage remark for %s: %s" % (kernel, r.stderr[-500:])
    assert len(scratch) == len(KERNELS), sorted(scratch)
    bad = [(n, scratch[n], spilled.get(n, 0)) for n in scratch if scratch[n] or spilled.get(n, 0)]
    assert not bad, "kernels spilling: %s" % bad
