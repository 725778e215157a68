#!/usr/bin/env python3
"""Times the hash-grid encoding (csrc/hashgrid.hip) next to the same encoding as a chain of PyTorch ops (tests/hashgrid_reference.py
op_chain) on the same GPU: the reference's default configuration (16 levels of 2 features, 2^19 rows a level, base 16, scale 1.4473),
N = 16 384 and 262 144 uniform points.  Timed: the forward; the forward with both backward passes; the three kernels one by one; and the
scatter's added bytes (N L 8 F 4) over its time, beside the two rates the microarchitecture notes give for float atomic adds (about
1.3 TB/s for wave-instructions of 256 contiguous bytes, about 0.08 TB/s with every lane in a different row).  Informational: nothing
asserts a ratio.

hipEvent timing around each call, warm-up runs first, the median of the timed runs.  Usage:
    python tools/bench_hashgrid.py [--sizes 16384 262144] [--runs 7] [--warmup 2] [--out profiles/hashgrid.txt]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIG = {"otype": "HashGrid", "n_levels": 16, "n_features_per_level": 2, "log2_hashmap_size": 19, "base_resolution": 16,
          "per_level_scale": 1.447269237440378}
SHAPED_TBS, SCATTERED_TBS = 1.3, 0.08


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


def main():
    import hashgrid_reference as reference
    from gaussianip_amd._lib import call_model, ptr
    from gaussianip_amd.utils.encoding import HashGridLayout, hash_grid_encode
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[16384, 262144])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hashgrid.txt"))
    args = ap.parse_args()
    layout = HashGridLayout(CONFIG)
    L, F = layout.n_levels, layout.n_features_per_level
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    table = ((torch.rand((layout.n_rows, F), device=dev, generator=gen) * 2 - 1) * 1e-1).requires_grad_(True)
    lines = ["tools/bench_hashgrid.py: L %d, F %d, 2^%d rows a level (%d rows, %.1f MB), base %d, scale %.4f; %d dense and %d hashed levels; "
             "%s (%s), median [min, max] of %d runs after %d warm-up, ms" % (
                 L, F, layout.log2_hashmap_size, layout.n_rows, layout.n_params * 4 / 1e6, layout.base_resolution, layout.per_level_scale,
                 layout.hashed.count(False), layout.hashed.count(True), torch.cuda.get_device_name(0),
                 torch.cuda.get_device_properties(0).gcnArchName, args.runs, args.warmup)]
    for N in args.sizes:
        x = torch.rand((N, 3), device=dev, generator=gen).requires_grad_(True)
        g = torch.randn((N, L * F), device=dev, generator=gen)
        xd, td = x.detach(), table.detach()
        enc, g_x, g_table = torch.empty((N, L * F), device=dev), torch.empty((N, 3), device=dev), torch.zeros_like(td)

        def kernel_forward():
            with torch.no_grad():
                return hash_grid_encode(xd, td, layout)

        def chain_forward():
            with torch.no_grad():
                return reference.op_chain(xd, td, layout)

        def kernel_both():
            return torch.autograd.grad((hash_grid_encode(x, table, layout) * g).sum(), (x, table))

        def chain_both():
            return torch.autograd.grad((reference.op_chain(x, table, layout) * g).sum(), (x, table))

        def only_forward():
            call_model(dev, "gip_hashgrid_forward", ptr(xd), ptr(td), *layout.level_args(N), ptr(enc))

        def only_backward_input():
            call_model(dev, "gip_hashgrid_backward_input", ptr(xd), ptr(td), ptr(g), *layout.level_args(N), ptr(g_x))

        def only_backward_table():                  # adds into the same buffer run after run: the values grow, the traffic does not
            call_model(dev, "gip_hashgrid_backward_table", ptr(xd), ptr(g), *layout.level_args(N), ptr(g_table))

        ke, ce = kernel_forward(), chain_forward()
        kg, cg = kernel_both(), chain_both()
        diff = [float((ke - ce).abs().max() / ce.abs().max())] + [float((a - b).abs().max() / b.abs().max()) for a, b in zip(kg, cg)]
        kf, cf = timed(kernel_forward, args.warmup, args.runs), timed(chain_forward, args.warmup, args.runs)
        kb, cb = timed(kernel_both, args.warmup, args.runs), timed(chain_both, args.warmup, args.runs)
        t_f, t_i, t_t = (timed(fn, args.warmup, args.runs) for fn in (only_forward, only_backward_input, only_backward_table))
        added = N * L * 8 * F * 4
        rate = added / (t_t[0] * 1e-3) / 1e12
        lines += ["N %7d" % N,
                  "       forward             kernels %9.3f [%.3f, %.3f]   op chain %9.3f [%.3f, %.3f]   ratio %.1fx" % (kf + cf + (cf[0] / kf[0],)),
                  "       forward + backward  kernels %9.3f [%.3f, %.3f]   op chain %9.3f [%.3f, %.3f]   ratio %.1fx" % (kb + cb + (cb[0] / kb[0],)),
                  "       gip_hashgrid_forward         %9.3f [%.3f, %.3f]" % t_f,
                  "       gip_hashgrid_backward_input  %9.3f [%.3f, %.3f]" % t_i,
                  "       gip_hashgrid_backward_table  %9.3f [%.3f, %.3f]" % t_t,
                  "       the scatter adds %.1f MB: %.3f TB/s of added bytes (shaped atomics %.2f TB/s would take %.3f ms, one row per lane "
                  "%.2f TB/s %.3f ms)" % (added / 1e6, rate, SHAPED_TBS, added / SHAPED_TBS / 1e9, SCATTERED_TBS, added / SCATTERED_TBS / 1e9),
                  "       max |kernel - chain| / max: enc %.2e, g_x %.2e, g_table %.2e" % tuple(diff)]
        del x, g, enc, g_x, g_table
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
