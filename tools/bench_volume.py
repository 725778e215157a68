#!/usr/bin/env python3
"""Times the volume-rendering kernels (csrc/volume.hip) next to the same compositing as a chain of PyTorch ops (tests/volume_reference.py
chain_weights / chain_accumulate: a segment cumsum and index_add_) on the same GPU.  The workload is the reference's own: 4 views of
64 x 64 rays, 512 steps across the box's diagonal, a 32^3 occupancy grid over [-1, 1]^3 with the sphere of radius 0.5 occupied; and the
same with an all-ones grid.  Timed: the march (two launches, a cumsum and the host read between them; the op chain has no march);
the weights forward, and forward with backward; the renderer's four accumulates (opacity, depth, colour, depth variance) forward, and
forward with backward; and each entry point alone on buffers made once, with the bytes it reads and writes over its time (the march's
bytes leave out the occupancy grid, 32 KB that stay in cache).  Informational: nothing asserts a ratio.

hipEvent timing around windows of --launches calls, warm-up windows first, kernels and op chain alternating, the median window over
its launches; the entry points alone take ten times as many calls a window.  Usage:
    python tools/bench_volume.py [--views 4] [--size 64] [--steps 512] [--launches 20] [--runs 9] [--warmup 2] [--out profiles/volume.txt]"""
import argparse
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def window(fn, launches):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(launches):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / launches


def timed(fns, launches, warmup, runs):
    """median [min, max] ms a call of every function of fns, their windows alternating."""
    for _ in range(warmup):
        for fn in fns:
            window(fn, launches)
    ms = [[] for _ in fns]
    for _ in range(runs):
        for k, fn in enumerate(fns):
            ms[k].append(window(fn, launches))
    return [(statistics.median(m), min(m), max(m)) for m in ms]


def look_at(position):
    p = torch.tensor(position, dtype=torch.float64)
    z = p / p.norm()
    x = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), z)
    x = x / x.norm()
    c2w = torch.eye(4, dtype=torch.float64)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, torch.linalg.cross(z, x), z, p
    return c2w.float()


def main():
    import volume_reference as reference
    from gaussianip_amd.utils import volume
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "volume.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    G, dt = 32, 1.732 * 2 / args.steps
    positions = [(2.5 * math.sin(a), 0.8, 2.5 * math.cos(a)) for a in (2 * math.pi * v / args.views for v in range(args.views))]
    rays_o, rays_d = volume.get_rays(volume.get_ray_directions(args.size, args.size, 1.2 * args.size), torch.stack([look_at(p) for p in positions]))
    rays_o, rays_d = rays_o.to(dev).contiguous(), rays_d.to(dev).contiguous()
    R = rays_o.shape[0]
    centres = (torch.arange(G, device=dev) + 0.5) / G * 2 - 1
    sphere = (centres[:, None, None] ** 2 + centres[None, :, None] ** 2 + centres[None, None, :] ** 2) <= 0.25
    lines = ["tools/bench_volume.py: %d views of %d x %d rays (%d), %d steps of %.5f, a %d^3 grid over [-1, 1]^3; %s (%s); median [min, max] "
             "of %d windows of %d calls after %d warm-up windows, ms a call" % (
                 args.views, args.size, args.size, R, args.steps, dt, G, torch.cuda.get_device_name(0),
                 torch.cuda.get_device_properties(0).gcnArchName, args.runs, args.launches, args.warmup)]
    chained = reference.Chained(torch.float32)
    for name, occ in (("sphere of radius 0.5 occupied", sphere), ("all-ones grid", torch.ones_like(sphere))):
        def march():
            return volume.march_rays(rays_o, rays_d, occ, [-1, -1, -1, 1, 1, 1], dt, max_samples_per_ray=args.steps + 1)
        idx, ts, te, offsets = march()
        M = int(idx.shape[0])
        per_ray = offsets[1:] - offsets[:-1]
        index = idx.long()
        t_mid = ((ts + te) / 2)[:, None]
        points = rays_o[index] + rays_d[index] * t_mid
        sigmas = (10.0 * torch.exp(-(points ** 2).sum(-1) / (2 * 0.3 ** 2))).requires_grad_(True)
        rgb = torch.sigmoid(points * 3).contiguous().requires_grad_(True)
        g_w = torch.randn(M, device=dev)
        g_out = [torch.randn((R, C), device=dev) for C in (1, 1, 3, 1)]

        def weights(fns, backward):
            def run():
                w = fns.render_weight_from_density(ts, te, sigmas, idx, R)[0]
                if backward:
                    torch.autograd.grad((w * g_w).sum(), sigmas)
            if backward:
                return run

            def forward():
                with torch.no_grad():
                    run()
            return forward

        w_leaf = volume.render_weight_from_density(ts, te, sigmas, idx, R)[0].detach().requires_grad_(True)
        depth = volume.accumulate_along_rays(w_leaf.detach(), t_mid, idx, R)
        spread = ((t_mid - depth[index]) ** 2).contiguous()

        def accumulates(fns, backward):
            def run():
                outs = [fns.accumulate_along_rays(w_leaf, v, idx, R) for v in (None, t_mid, rgb, spread)]
                if backward:
                    torch.autograd.grad(sum((o * g).sum() for o, g in zip(outs, g_out)), (w_leaf, rgb))
                return outs
            if backward:
                return run

            def forward():
                with torch.no_grad():
                    return run()
            return forward

        ko, co = accumulates(volume, False)(), accumulates(chained, False)()
        kw, cw = volume.render_weight_from_density(ts, te, sigmas, idx, R)[0], chained.render_weight_from_density(ts, te, sigmas, idx, R)[0]
        diff = [float((kw - cw).detach().abs().max() / cw.detach().abs().max())] + [float((a - b).abs().max() / b.abs().max()) for a, b in zip(ko, co)]
        (t_march,) = timed([march], max(args.launches // 4, 1), args.warmup, args.runs)
        rows = [("weights forward", weights(volume, False), weights(chained, False)),
                ("weights forward + backward", weights(volume, True), weights(chained, True)),
                ("4 accumulates forward", accumulates(volume, False), accumulates(chained, False)),
                ("4 accumulates forward + backward", accumulates(volume, True), accumulates(chained, True))]
        lines += ["%s: %d samples, %d rays with samples, at most %d a ray, mean %.1f over those" % (
                      name, M, int((per_ray > 0).sum()), int(per_ray.max()), M / max(int((per_ray > 0).sum()), 1)),
                  "       %-34s kernels %9.3f [%.3f, %.3f]   (count, cumsum, host read, emit; no op chain)" % (("march",) + t_march)]
        for label, kernel_fn, chain_fn in rows:
            k, c = timed([kernel_fn, chain_fn], args.launches, args.warmup, args.runs)
            lines.append("       %-34s kernels %9.3f [%.3f, %.3f]   op chain %9.3f [%.3f, %.3f]   ratio %.1fx" % ((label,) + k + c + (c[0] / k[0],)))
        # the entry points alone, on buffers made once: what the kernels take without the Python surface around them
        from gaussianip_amd._lib import call_model, ptr
        grid8 = occ.contiguous().view(torch.uint8)
        box = (-1.0, -1.0, -1.0, 1.0, 1.0, 1.0) + (G / 2.0,) * 3 + (dt, 0.0, 1e10, args.steps + 1)
        counts = torch.empty(R, dtype=torch.int32, device=dev)
        bufs = [torch.empty(M, device=dev) for _ in range(4)]
        sg, rgb_d, wl = sigmas.detach(), rgb.detach(), w_leaf.detach()
        out3, g_v3 = torch.empty((R, 3), device=dev), torch.empty((M, 3), device=dev)
        idx_out = torch.empty(M, dtype=torch.int32, device=dev)
        alone = [("gip_volume_march_count", R * 28, lambda: call_model(dev, "gip_volume_march_count", ptr(rays_o), ptr(rays_d), ptr(grid8), ptr(None), R, G,
                                                                      *box, ptr(counts))),
                 ("gip_volume_march_emit", R * 28 + M * 12, lambda: call_model(dev, "gip_volume_march_emit", ptr(rays_o), ptr(rays_d), ptr(grid8), ptr(None),
                                                                              R, G, *box, ptr(offsets), M, ptr(idx_out), ptr(bufs[0]), ptr(bufs[1]))),
                 ("gip_volume_weights_forward", M * 24, lambda: call_model(dev, "gip_volume_weights_forward", ptr(ts), ptr(te), ptr(sg), ptr(offsets), R, M,
                                                                          ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]))),
                 ("gip_volume_weights_backward", M * 28, lambda: call_model(dev, "gip_volume_weights_backward", ptr(ts), ptr(te), ptr(g_w), ptr(bufs[0]),
                                                                           ptr(bufs[1]), ptr(bufs[2]), ptr(offsets), R, M, ptr(bufs[3]))),
                 ("gip_volume_accumulate_forward C 3", M * 16 + R * 12, lambda: call_model(dev, "gip_volume_accumulate_forward", ptr(wl), ptr(rgb_d), ptr(offsets),
                                                                                          R, M, 3, ptr(out3))),
                 ("gip_volume_accumulate_backward C 3", M * 36, lambda: call_model(dev, "gip_volume_accumulate_backward", ptr(wl), ptr(rgb_d), ptr(idx),
                                                                                  ptr(g_out[2]), R, M, 3, ptr(bufs[3]), ptr(g_v3)))]
        for (label, nbytes, _), t in zip(alone, timed([fn for _, _, fn in alone], 10 * args.launches, args.warmup, args.runs)):
            lines.append("       %-34s alone   %9.4f [%.4f, %.4f]   %6.1f MB read and written, %.3f TB/s" % (
                (label,) + t + (nbytes / 1e6, nbytes / (t[0] * 1e-3) / 1e12)))
        lines.append("       max |kernel - chain| / max: weights %.2e, opacity %.2e, depth %.2e, colour %.2e, variance %.2e" % tuple(diff))
        del sigmas, rgb, g_w, g_out, w_leaf, points, spread
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
