#!/usr/bin/env python3
"""Times the NeuS rendering of a signed-distance field (csrc/volume_sdf.hip): the fused call render_sdf_rays (one launch forward, one
backward) next to the op chain on the same samples, which is what NeuSVolumeRenderer(fused=False) runs: neus_alpha as PyTorch ops, then
render_weight_from_alpha and three accumulate_along_rays calls, each an autograd.Function with its own host path.  The workload is
the reference's own: 4 views of 64 x 64 rays, 512 steps across the box's diagonal, a 32^3 occupancy grid over [-1, 1]^3 with the cells
within 0.1 of the sphere of radius 0.5 occupied, the SDF of that sphere, its normals, a colour per sample, beta = exp(3).  Timed: the
forward, and forward with backward (gradients to sdf, normals, colour and inv_std); and each entry point alone on buffers made once,
with the bytes it reads and writes over its time.  Informational: nothing asserts a ratio.

hipEvent timing around windows of --launches calls, warm-up windows first, the two alternating, the median window over its launches;
the entry points alone take ten times as many calls a window.  Usage:
    python tools/bench_sdf_volume.py [--views 4] [--size 64] [--steps 512] [--launches 20] [--runs 9] [--warmup 2] [--out profiles/sdf_volume.txt]"""
import argparse
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    from bench_volume import look_at, timed
    from gaussianip_amd._lib import call_model, ptr
    from gaussianip_amd.utils import sdf_volume, volume
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdf_volume.txt"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    G, dt, radius = 32, 1.732 * 2 / args.steps, 0.5
    positions = [(2.5 * math.sin(a), 0.8, 2.5 * math.cos(a)) for a in (2 * math.pi * v / args.views for v in range(args.views))]
    rays_o, rays_d = volume.get_rays(volume.get_ray_directions(args.size, args.size, 1.2 * args.size), torch.stack([look_at(p) for p in positions]))
    rays_o, rays_d = rays_o.to(dev).contiguous(), rays_d.to(dev).contiguous()
    R = rays_o.shape[0]
    centres = (torch.arange(G, device=dev) + 0.5) / G * 2 - 1
    dist = torch.sqrt(centres[:, None, None] ** 2 + centres[None, :, None] ** 2 + centres[None, None, :] ** 2)
    lines = ["tools/bench_sdf_volume.py: %d views of %d x %d rays (%d), %d steps of %.5f, a %d^3 grid over [-1, 1]^3, a sphere SDF of radius %.1f, "
             "beta = exp(3); %s (%s); median [min, max] of %d windows of %d calls after %d warm-up windows, ms a call" % (
                 args.views, args.size, args.size, R, args.steps, dt, G, radius, torch.cuda.get_device_name(0),
                 torch.cuda.get_device_properties(0).gcnArchName, args.runs, args.launches, args.warmup)]
    for name, occ in (("shell within 0.1 of the sphere occupied", (dist - radius).abs() <= 0.1), ("ball of radius 0.6 occupied", dist <= 0.6)):
        idx, ts, te, offsets = volume.march_rays(rays_o, rays_d, occ, [-1, -1, -1, 1, 1, 1], dt, max_samples_per_ray=args.steps + 1)
        M = int(idx.shape[0])
        per_ray = offsets[1:] - offsets[:-1]
        index = idx.long()
        t_mid = ((ts + te) / 2)[:, None].contiguous()
        points = rays_o[index] + rays_d[index] * t_mid
        norm = points.norm(dim=-1, keepdim=True)
        sdf = (norm[:, 0] - radius).contiguous().requires_grad_(True)
        normals = (points / norm).contiguous().requires_grad_(True)
        rgb = torch.sigmoid(points * 3).contiguous().requires_grad_(True)
        log_beta = torch.tensor(0.3, device=dev, requires_grad=True)
        t_dirs, t_intervals = rays_d[index], te - ts
        g_out, g_w = torch.randn((R, 5), device=dev), torch.randn(M, device=dev)
        leaves = (sdf, normals, rgb, log_beta)

        def fused():
            inv_std = torch.exp(log_beta * 10.0).clamp(1e-6, 1e6).reshape(1)
            out, weights, _ = sdf_volume.render_sdf_rays(sdf, normals, rays_d, ts, te, rgb, inv_std, idx, R, 1.0)
            return out, weights

        def chain():
            inv_std = torch.exp(log_beta * 10.0).clamp(1e-6, 1e6)
            alpha = sdf_volume.neus_alpha(sdf, normals, t_dirs, t_intervals, torch.ones_like(sdf) * inv_std, 1.0)
            weights, _ = sdf_volume.render_weight_from_alpha(alpha, idx, R)
            out = torch.cat((volume.accumulate_along_rays(weights, None, idx, R), volume.accumulate_along_rays(weights, t_mid, idx, R),
                             volume.accumulate_along_rays(weights, rgb, idx, R)), dim=1)
            return out, weights

        def forward(fn):
            def run():
                with torch.no_grad():
                    fn()
            return run

        def both(fn):
            def run():
                out, weights = fn()
                torch.autograd.grad((out * g_out).sum() + (weights * g_w).sum(), leaves)
            return run

        (fo, fw), (co, cw) = fused(), chain()
        diff = [float((fw - cw).detach().abs().max() / cw.detach().abs().max())] + [
            float((fo[:, a:b] - co[:, a:b]).detach().abs().max() / co[:, a:b].detach().abs().max()) for a, b in ((0, 1), (1, 2), (2, 5))]
        lines.append("%s: %d samples, %d rays with samples, at most %d a ray, mean %.1f over those" % (
            name, M, int((per_ray > 0).sum()), int(per_ray.max()), M / max(int((per_ray > 0).sum()), 1)))
        for label, wrap in (("forward", forward), ("forward + backward", both)):
            k, c = timed([wrap(fused), wrap(chain)], args.launches, args.warmup, args.runs)
            slower = "   FUSED IS SLOWER" if k[0] > c[0] else ""
            lines.append("       %-34s fused   %9.3f [%.3f, %.3f]   op chain %9.3f [%.3f, %.3f]   ratio %.1fx%s" % ((label,) + k + c + (c[0] / k[0], slower)))
        # the entry points alone, on buffers made once: what the kernels take without the Python surface around them
        s, n, v = sdf.detach(), normals.detach(), rgb.detach()
        beta = torch.tensor([math.exp(3.0)], device=dev)
        alphas, trans, weights, g_a, g_s = (torch.empty(M, device=dev) for _ in range(5))
        out, g_n, g_v, g_rays = torch.empty((R, 5), device=dev), torch.empty((M, 3), device=dev), torch.empty((M, 3), device=dev), torch.empty(R, device=dev)
        common = (ptr(s), ptr(n), ptr(rays_d), ptr(ts), ptr(te), ptr(v), ptr(offsets), ptr(beta), 1.0)
        call_model(dev, "gip_volume_sdf_render_forward", *common, R, M, 3, ptr(alphas), ptr(trans), ptr(weights), ptr(out))
        alone = [("gip_volume_sdf_render_forward C 3", M * 48 + R * 36, lambda: call_model(dev, "gip_volume_sdf_render_forward", *common, R, M, 3, ptr(alphas),
                                                                                          ptr(trans), ptr(weights), ptr(out))),
                 ("gip_volume_sdf_render_backward C 3", M * 80 + R * 36, lambda: call_model(dev, "gip_volume_sdf_render_backward", *common, ptr(alphas), ptr(trans),
                                                                                           ptr(weights), ptr(g_out), ptr(g_w), R, M, 3, ptr(g_s), ptr(g_n),
                                                                                           ptr(g_v), ptr(g_rays))),
                 ("gip_volume_alpha_weights_forward", M * 12, lambda: call_model(dev, "gip_volume_alpha_weights_forward", ptr(alphas), ptr(offsets), R, M,
                                                                                ptr(weights), ptr(trans))),
                 ("gip_volume_alpha_weights_backward", M * 16, lambda: call_model(dev, "gip_volume_alpha_weights_backward", ptr(alphas), ptr(trans), ptr(g_w),
                                                                                 ptr(offsets), R, M, ptr(g_a)))]
        for (label, nbytes, _), t in zip(alone, timed([fn for _, _, fn in alone], 10 * args.launches, args.warmup, args.runs)):
            lines.append("       %-34s alone   %9.4f [%.4f, %.4f]   %6.1f MB read and written, %.3f TB/s" % (
                (label,) + t + (nbytes / 1e6, nbytes / (t[0] * 1e-3) / 1e12)))
        lines.append("       max |fused - chain| / max: weights %.2e, opacity %.2e, depth %.2e, colour %.2e" % tuple(diff))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
