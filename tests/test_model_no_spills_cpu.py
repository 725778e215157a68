"""No kernel of libgip_model.so's sources listed below may use scratch memory or spill registers: each file is compiled with the
Makefile's flags of that library (-ffp-contract=off) and the compiler's kernel-resource-usage remarks are read.  Every named kernel
must be found, the file must hold no other kernel, and nothing is allowed to spill.  What each file keeps per lane, which is what
would spill first:
  field.hip            the evaluate kernel keeps up to 16 voxels with three coordinates, an address, a sum and a batch sum each; it also
                       holds the one prepare kernel of the field family, which the next two files launch through a host function.
  field_sample.hip     the evaluate kernel keeps SAMPLE_PPT points with seven sums and seven batch sums each.
  texture.hip          the evaluate kernel keeps TEX_PPT texels with three coordinates, four sums and four batch sums each.
                       (The per-lane arrays of these three are handed to the shared walk of field_common.h by reference.)
  texture_project.hip  the kernel keeps a texel's point, normal and four sums and loops over the views without a local array.
  mesh_raster.hip      the set-up kernel keeps a triangle's snapped corners, three 64-bit edge functions and their six 64-bit steps.
  mesh_grad.hip        the antialias kernels keep what four pixel pairs found (weight, edge, slope), in arrays that must stay in registers.
  mesh_mip.hip         the lookup's backward keeps two levels' taps and weights.
tests/test_no_kernel_spills_cpu.py does the same for libgip_raster.so, with that library's flags and an allow-list."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussianip_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SOURCES = [
    ("field.hip", ("field_prepare_kernel", "field_eval_kernelILi1E", "field_eval_kernelILi2E", "field_eval_kernelILi4E", "field_eval_kernelILi8E",
                   "field_eval_kernelILi16E", "surface_count_kernel", "surface_emit_kernel")),
    ("field_sample.hip", ("sample_eval_kernelILi4ELb0E", "sample_eval_kernelILi4ELb1E")),
    ("ssim.hip", ("ssim_forward_kernel", "ssim_backward_kernel", "ssim_finish_kernel")),
    ("texture.hip", ("texture_eval_kernelILi4EE",)),
    ("texture_project.hip", ("texture_project_kernel",)),
    ("mesh_raster.hip", ("mesh_setup_kernel", "mesh_large_kernel", "mesh_resolve_kernel", "mesh_shade_kernel", "mesh_shade_backward_kernel",
                         "mesh_interpolate_kernel", "mesh_interpolate_backward_kernel", "mesh_texture_kernel", "mesh_texture_backward_kernel")),
    ("mesh_grad.hip", ("mesh_rasterize_backward_kernel", "mesh_interpolate_backward_rast_kernel", "mesh_shade_backward_rast_kernel",
                       "mesh_antialias_kernel", "mesh_antialias_backward_kernel")),
    ("mesh_mip.hip", ("mesh_rast_db_kernel", "mesh_interpolate_da_kernel", "mesh_interpolate_da_backward_kernel", "mesh_mip_build_kernel",
                      "mesh_mip_fold_kernel", "mesh_texture_mip_kernel", "mesh_texture_mip_backward_kernel")),
    ("mesh_clean.hip", ("mc_hook_kernel", "mc_compress_kernel", "mc_stats_init_kernel", "mc_stats_kernel", "mc_box_decode_kernel", "mc_keys_kernel",
                        "mc_count_kernel", "mc_place_kernelILi16E", "mc_place_kernelILi32E", "mc_place_kernelILi64E")),
]


def resource_usage(source, out):
    """({kernel: scratch bytes per lane}, {kernel: SGPRs + VGPRs spilled}, the compiler's remarks) of one file of csrc/."""
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
           "-ffp-contract=off", "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", os.path.join(CSRC, source),
           "-o", str(out)]
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
    return scratch, spilled, r.stderr


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("source,kernels", SOURCES, ids=[s for s, _ in SOURCES])
def test_model_kernels_do_not_spill(tmp_path, source, kernels):
    scratch, spilled, log = resource_usage(source, tmp_path / "o.o")
    for kernel in kernels:
        assert any(kernel in n for n in scratch), "no kernel-resource-usage remark for %s: %s" % (kernel, log[-500:])
    assert len(scratch) == len(kernels), sorted(scratch)
    bad = [(n, scratch[n], spilled.get(n, 0)) for n in scratch if scratch[n] or spilled.get(n, 0)]
    assert not bad, "kernels spilling: %s" % bad
