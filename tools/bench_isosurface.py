#!/usr/bin/env python3
"""Times marching_tetrahedra (csrc/mesh_tets.hip) forward and forward + backward next to the same surface as the reference's chain of
PyTorch ops (tests/isosurface_reference.py, which sorts on every call) on the same GPU: Kuhn grids at R = 64 (1.57 M tetrahedra, about
the size of the reference's 128-grid) and R = 128, the distance of a sphere of radius 0.3, gradients to the distance and to a
deformation.  Informational: nothing asserts a ratio.

hipEvent timing around each call, warm-up runs first, the median of the timed runs.  The launches and host synchronisations of one
forward + backward call are counted with torch.profiler (device kernels and copies; runtime calls that wait for the device).  Usage:
    python tools/bench_isosurface.py [--resolutions 64 128] [--runs 7] [--warmup 2] [--out profiles/isosurface.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, warmup, runs):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return statistics.median(ms), min(ms), max(ms)


def counted(fn):
    """(device kernels and copies, host calls that wait for the device) of one call of fn, or None where the profiler gives nothing."""
    from torch.profiler import ProfilerActivity, profile
    try:
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        device = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
        waits = sum(1 for e in prof.events() if not str(e.device_type).endswith("CUDA") and
                    (("Synchronize" in e.name and e.name.startswith(("hip", "cuda"))) or
                     (e.name.startswith(("hipMemcpy", "cudaMemcpy")) and "Async" not in e.name)))
        return device, waits - 1                             # the synchronize above is not the call's own
    except Exception as exc:                                 # noqa: BLE001  the count is a convenience, the timing is the tool
        print("profiler unavailable: %s" % exc)
        return None


def main():
    import isosurface_reference as reference
    from gaussianip_amd.utils.isosurface import TetGrid, marching_tetrahedra
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "isosurface.txt"))
    args = ap.parse_args()
    lines = ["tools/bench_isosurface.py: Kuhn grids, sphere of radius 0.3, %s (%s), median [min, max] of %d runs after %d warm-up, ms" % (
        torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName, args.runs, args.warmup)]
    for R in args.resolutions:
        grid = TetGrid.kuhn(R, device="cuda")
        sdf = ((grid.vertices - 0.5).norm(dim=1) - 0.3).requires_grad_(True)
        deformation = torch.zeros_like(grid.vertices).requires_grad_(True)
        tets = grid.indices.long()

        def positions():
            return grid.vertices + torch.tanh(deformation) / R

        def kernel_forward():
            with torch.no_grad():
                return marching_tetrahedra(grid, sdf, positions())

        def chain_forward():
            with torch.no_grad():
                return reference.marching_tetrahedra(positions(), sdf, tets)

        def kernel_both():
            v, _ = marching_tetrahedra(grid, sdf, positions())
            return torch.autograd.grad(v.sum(), (sdf, deformation))

        def chain_both():
            v, _ = reference.marching_tetrahedra(positions(), sdf, tets)
            return torch.autograd.grad(v.sum(), (sdf, deformation))

        (v, f), (rv, rf) = kernel_forward(), chain_forward()
        same = bool(torch.equal(f.long(), rf)) and v.shape == rv.shape
        diff = float((v - rv).abs().max()) if same else float("nan")
        g, rg = kernel_both(), chain_both()
        gdiff = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(g, rg)]
        kf, cf = timed(kernel_forward, args.warmup, args.runs), timed(chain_forward, args.warmup, args.runs)
        kb, cb = timed(kernel_both, args.warmup, args.runs), timed(chain_both, args.warmup, args.runs)
        kc, cc = counted(kernel_both), counted(chain_both)
        lines += ["R %3d  %d grid vertices, %d tetrahedra, %d edges; surface %d vertices, %d faces" % (
                      R, grid.num_vertices, grid.num_tets, grid.num_edges, v.shape[0], f.shape[0]),
                  "       forward             kernels %9.3f [%.3f, %.3f]   op chain %9.3f [%.3f, %.3f]   ratio %.1fx" % (kf + cf + (cf[0] / kf[0],)),
                  "       forward + backward  kernels %9.3f [%.3f, %.3f]   op chain %9.3f [%.3f, %.3f]   ratio %.1fx" % (kb + cb + (cb[0] / kb[0],)),
                  "       faces identical: %s   max |kernel - chain| of the vertices %.2e   of the gradients / max: sdf %.2e, deformation %.2e" % (
                      same, diff, gdiff[0], gdiff[1])]
        if kc and cc:
            lines.append("       one forward + backward: kernels path %d device launches and copies, %d host waits; op chain %d and %d" % (kc + cc))
        del grid, tets
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
