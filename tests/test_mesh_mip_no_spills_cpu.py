"""No kernel of csrc/mesh_mip.hip may spill registers to scratch memory: the compile line and the parsing of
tests/test_mesh_grad_no_spills_cpu.py (the Makefile's flags of libgip_model.so: -ffp-contract=off), nothing allowed to spill, and the
number of kernels exact.  The lookup's backward keeps two levels' taps and weights per lane."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussianip_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ("mesh_rast_db_kernel", "mesh_interpolate_da_kernel", "mesh_interpolate_da_backward_kernel", "mesh_mip_build_kernel",
           "mesh_mip_fold_kernel", "mesh_texture_mip_kernel", "mesh_texture_mip_backward_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_mesh_mip_kernels_do_not_spill(tmp_path):
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", os.path.join(CSRC, "mesh_mip.hip"),
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
