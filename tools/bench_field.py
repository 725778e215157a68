#!/usr/bin/env python3
"""Times GaussianModel.extract_fields and extract_mesh (csrc/field.hip) on 100k Gaussians of the human-shaped cloud of tests/scenes.py
at 128^3 and 256^3, next to the same field written as the reference's block loop of PyTorch ops on the same GPU (this file's own
statement of that op chain: one masked gather and a [voxels, members] evaluation per block, Gaussians in batches of 1024).

hipEvent timing around each call, warm-up runs first, the median of the timed runs.  Usage:
    python tools/bench_field.py [--points 100000] [--runs 7] [--warmup 2] [--chain-runs 3] [--out profiles/field_extract.txt]
    python tools/bench_field.py --once 128      one extract_fields + extract_mesh call (for a kernel trace)
    python tools/bench_field.py --attributes    extract_mesh_with_attributes (csrc/field_sample.hip) next to extract_mesh at the default
                                                geometry (R 128, 16 blocks), and the same three sums at the same vertices as a
                                                chunked dense evaluation in PyTorch ops (--out defaults to profiles/field_sample.txt)
    python tools/bench_field.py --texture       bake_texture (csrc/texture.hip) on the mesh of R 128 / 16 blocks at the default texture
                                                size and at 2048: the whole call, gip_texture_bake alone, and the route without it on
                                                the same texels — texel_points materialised, sorted by block, gip_field_sample, the
                                                sums scattered into the texture (--out defaults to profiles/texture_bake.txt)
    python tools/bench_field.py --decimate      clean_mesh and decimate_mesh (csrc/mesh_clean.hip) on the mesh of R 128 / 16 blocks: the
                                                cleaning, the decimation to 1e5 and to 2e4 faces, the placement kernel alone at 16, 32
                                                and 64 lanes per cell, and the atlas cell at T = 4096 before and after (--out defaults to
                                                profiles/mesh_clean.txt)"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def make_model(P):
    import scenes
    from gaussianip_amd.scene import GaussianModel
    sc = scenes.trained_look(scenes.make_scene("human", P, seed=42))
    gm = GaussianModel(0)
    gm._xyz = torch.from_numpy(sc["means3D"]).cuda()
    gm._opacity = torch.logit(torch.from_numpy(sc["opacities"])).cuda()
    gm._scaling = torch.log(torch.from_numpy(sc["scales"])).cuda()
    gm._rotation = torch.from_numpy(sc["rotations"]).cuda()
    return gm


@torch.no_grad()
def op_chain(gm, resolution, num_blocks=16, relax_ratio=1.5, count_pairs=False):
    """The field as a loop over blocks of PyTorch ops (the form the reference computes it in)."""
    from gaussianip_amd.utils.general import build_scaling_rotation
    dev = gm._xyz.device
    opac = torch.sigmoid(gm._opacity)
    keep = (opac > 0.005).squeeze(1)
    opac, xyz, std, rot = opac[keep], gm._xyz[keep], torch.exp(gm._scaling[keep]), gm._rotation[keep]
    mn, mx = xyz.amin(0), xyz.amax(0)
    center, scale = (mn + mx) / 2, 1.8 / (mx - mn).amax().item()
    xyz, std = (xyz - center) * scale, std * scale
    L = build_scaling_rotation(std, rot)
    S = L @ L.transpose(1, 2)
    a, b, c, d, e, f = S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]
    inv_det = 1 / (a * d * f + 2 * e * c * b - e ** 2 * a - c ** 2 * d - b ** 2 * f + 1e-24)
    inv = torch.stack(((d * f - e ** 2) * inv_det, (e * c - b * f) * inv_det, (e * b - c * d) * inv_det, (a * f - c ** 2) * inv_det,
                       (b * c - e * a) * inv_det, (a * d - b ** 2) * inv_det), 1)
    occ = torch.zeros((resolution,) * 3, device=dev)
    pairs = 0
    s, margin = resolution // num_blocks, (2 / num_blocks) * relax_ratio
    parts = torch.linspace(-1, 1, resolution).to(dev).split(s)
    for xi, xs in enumerate(parts):
        for yi, ys in enumerate(parts):
            for zi, zs in enumerate(parts):
                lo = torch.stack((xs[0], ys[0], zs[0])) - margin
                hi = torch.stack((xs[-1], ys[-1], zs[-1])) + margin
                m = (xyz < hi).all(-1) & (xyz > lo).all(-1)
                if not m.any():
                    continue
                pairs += int(m.sum()) * s ** 3 if count_pairs else 0
                pts = torch.stack(torch.meshgrid(xs, ys, zs, indexing="ij"), -1).reshape(-1, 3)
                mx_, mi, mo = xyz[m], inv[m], opac[m].view(1, -1)
                val = 0
                for st in range(0, mx_.shape[0], 1024):
                    g = pts.unsqueeze(1) - mx_[st:st + 1024].unsqueeze(0)
                    x, y, z = g[..., 0], g[..., 1], g[..., 2]
                    q = mi[st:st + 1024]
                    power = -0.5 * (x ** 2 * q[:, 0] + y ** 2 * q[:, 3] + z ** 2 * q[:, 5]) - x * y * q[:, 1] - x * z * q[:, 2] - y * z * q[:, 4]
                    power = torch.where(power > 0, torch.full_like(power, -1e10), power)
                    val = val + (mo[:, st:st + 1024] * torch.exp(power)).sum(-1)
                occ[xi * s:xi * s + s, yi * s:yi * s + s, zi * s:zi * s + s] = val.reshape(s, s, s)
    return (occ, pairs) if count_pairs else occ


@torch.no_grad()
def dense_sample(gm, u, block, rgb, resolution=128, num_blocks=16, relax_ratio=1.5, chunk=1024):
    """density, gradient and colour sum at the normalised points u, point i in block[i], as PyTorch ops: every point of a chunk
    meets every Gaussian and non-members are masked (this file's statement of what csrc/field_sample.hip computes)."""
    from gaussianip_amd.utils.general import build_scaling_rotation
    dev = gm._xyz.device
    opac = torch.sigmoid(gm._opacity)
    keep = (opac > 0.005).squeeze(1)
    opac, xyz, std, rot, rgb = opac[keep].view(1, -1), gm._xyz[keep], torch.exp(gm._scaling[keep]), gm._rotation[keep], rgb[keep]
    mn, mx = xyz.amin(0), xyz.amax(0)
    center, scale = (mn + mx) / 2, 1.8 / (mx - mn).amax().item()
    xyz, std = (xyz - center) * scale, std * scale
    L = build_scaling_rotation(std, rot)
    S = L @ L.transpose(1, 2)
    a, b, c, d, e, f = S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]
    inv_det = 1 / (a * d * f + 2 * e * c * b - e ** 2 * a - c ** 2 * d - b ** 2 * f + 1e-24)
    ia, ib, ic = (d * f - e ** 2) * inv_det, (e * c - b * f) * inv_det, (e * b - c * d) * inv_det
    id_, ie, if_ = (a * f - c ** 2) * inv_det, (b * c - e * a) * inv_det, (a * d - b ** 2) * inv_det
    s, margin = resolution // num_blocks, (2 / num_blocks) * relax_ratio
    grid = torch.linspace(-1, 1, resolution).to(dev)
    lo, hi = grid[0::s] - margin, grid[s - 1::s] + margin
    inside = (xyz.unsqueeze(-1) > lo) & (xyz.unsqueeze(-1) < hi)                      # [P, 3, nb]
    bx, by, bz = block // (num_blocks * num_blocks), (block // num_blocks) % num_blocks, block % num_blocks
    dens, grad, csum = [], [], []
    for st in range(0, u.shape[0], chunk):
        sl = slice(st, st + chunk)
        m = (inside[:, 0, bx[sl]] & inside[:, 1, by[sl]] & inside[:, 2, bz[sl]]).t()  # [v, P]
        x, y, z = (u[sl, k:k + 1] - xyz[:, k].unsqueeze(0) for k in range(3))
        power = -0.5 * (x ** 2 * ia + y ** 2 * id_ + z ** 2 * if_) - x * y * ib - x * z * ic - y * z * ie
        w = torch.where(m & ~(power > 0), opac * torch.exp(power.clamp_max(0)), torch.zeros_like(power))
        dens.append(w.sum(1))
        grad.append(torch.stack(((w * -(ia * x + ib * y + ic * z)).sum(1), (w * -(ib * x + id_ * y + ie * z)).sum(1),
                                 (w * -(ic * x + ie * y + if_ * z)).sum(1)), 1))
        csum.append(w @ rgb)
    return torch.cat(dens), torch.cat(grad), torch.cat(csum)


def attributes(gm, args):
    """extract_mesh, extract_mesh_with_attributes and the dense PyTorch evaluation at the default geometry."""
    from gaussianip_amd.utils import mesh
    R, nb = 128, 16
    rgb = torch.rand(gm._xyz.shape[0], 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    v, f, n, c = gm.extract_mesh_with_attributes(resolution=R, num_blocks=nb, colors=rgb)
    idx, _ = mesh.extract_surface(gm.extract_fields(resolution=R, num_blocks=nb), 1.0)       # the vertices in grid-index units
    u = idx / (R - 1.0) * 2 - 1
    cell = idx.floor().long().clamp(0, R - 1) // (R // nb)
    block = (cell[:, 0] * nb + cell[:, 1]) * nb + cell[:, 2]
    occupied = int(torch.unique(block).numel())
    dens, grad, csum = dense_sample(gm, u, block, rgb, R, nb)
    got = gm._sample("bench_field", u, block, rgb, R, nb, 1.5)
    diffs = [float((got[k] - ref).abs().max() / ref.abs().max()) for k, ref in (("density", dens), ("gradient", grad), ("color_sum", csum))]
    m = timed(lambda: gm.extract_mesh(resolution=R, num_blocks=nb), args.warmup, args.runs)
    a = timed(lambda: gm.extract_mesh_with_attributes(resolution=R, num_blocks=nb, colors=rgb), args.warmup, args.runs)
    k = timed(lambda: gm._sample("bench_field", u, block, rgb, R, nb, 1.5), args.warmup, args.runs)
    t = timed(lambda: dense_sample(gm, u, block, rgb, R, nb), 1, args.chain_runs)
    return ["R %3d  extract_mesh %9.3f [%.3f, %.3f]   extract_mesh_with_attributes %9.3f [%.3f, %.3f]" % ((R,) + m + a),
            "       %d vertices, %d faces, %d of %d blocks hold a vertex" % (v.shape[0], f.shape[0], occupied, nb ** 3),
            "       sampling alone (sort by block + gip_field_sample) %9.3f [%.3f, %.3f]" % k,
            "       dense PyTorch evaluation at the same vertices %9.3f [%.3f, %.3f] (%d runs)   ratio to sampling %.1fx" % (
                t + (args.chain_runs, t[0] / k[0])),
            "       max |kernel - dense| / max: density %.2e, gradient %.2e, color_sum %.2e" % tuple(diffs)]


def texture(gm, args):
    """bake_texture, its C entry point alone and the sampler's route on the same texels, at the default texture size and at 2048."""
    import ctypes

    from gaussianip_amd import _lib
    from gaussianip_amd.utils import texture as tex
    R, nb = 128, 16
    rgb = torch.rand(gm._xyz.shape[0], 3, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    v, f = gm.extract_mesh(resolution=R, num_blocks=nb)
    F = int(f.shape[0])
    lines = ["R %3d  %d vertices, %d faces" % (R, v.shape[0], F)]
    for T in (gm._default_texture_size(F), 2048):
        c = tex.atlas_layout(F, T)[0]
        _, xyzs, opac, stds, rots = gm._field_sources()
        mask = (gm.get_opacity > 0.005).squeeze(1)
        cols = rgb[mask].contiguous()
        u = ((v - gm.center) * gm.scale).contiguous()
        tri = u[f.long()]
        grid = torch.linspace(-1, 1, R, dtype=torch.float32).cuda()
        cell = (torch.bucketize(((tri[:, 0] + tri[:, 1] + tri[:, 2]) / 3).contiguous(), grid, right=True) - 1).clamp(0, R - 1) // (R // nb)
        block = (cell[:, 0] * nb + cell[:, 1]) * nb + cell[:, 2]
        counts = torch.bincount(block, minlength=nb ** 3)
        order = torch.sort(block, stable=True).indices.to(torch.int32)
        start = torch.cat((counts.new_zeros(1), counts.cumsum(0))).to(torch.int32)
        slices = min(max((int(counts.max()) * (c * (c + 1) // 2) + 1023) // 1024, 1), 1024)
        P = int(opac.shape[0])
        need = ctypes.c_size_t(0)
        lib = _lib.model_lib()
        assert lib.gip_texture_bake_workspace_size(P, R, nb, ctypes.byref(need)) == 0
        ws = torch.empty(need.value, dtype=torch.uint8, device="cuda")
        dens, csum = torch.zeros((T, T), device="cuda"), torch.zeros((T, T, 3), device="cuda")
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        center = gm.center.contiguous()

        def kernel():
            rc = lib.gip_texture_bake(p(xyzs), p(opac), p(stds), p(rots), p(cols), P, p(center), gm.scale, p(grid), R, nb, (2 / nb) * 1.5,
                                      p(u), int(u.shape[0]), p(f), F, p(order), p(start), T, c, slices, p(ws), need.value, p(dens), p(csum),
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, rc

        def route():
            pts, face, x, y = tex.texel_points(u, f, T)
            out = gm._sample("bench_field", pts.contiguous(), block[face], rgb, R, nb, 1.5)
            d, cs = torch.zeros((T, T), device="cuda"), torch.zeros((T, T, 3), device="cuda")
            d[y, x], cs[y, x] = out["density"], out["color_sum"]
            return d, cs

        # texel-Gaussian pairs: every owned texel meets every member of its face's block
        s_, margin = R // nb, (2 / nb) * 1.5
        xn = (xyzs - gm.center) * gm.scale
        inside = ((xn.unsqueeze(-1) > grid[0::s_] - margin) & (xn.unsqueeze(-1) < grid[s_ - 1::s_] + margin)).float()      # [P, 3, nb]
        members = torch.einsum("pa,pb,pc->abc", inside[:, 0], inside[:, 1], inside[:, 2]).reshape(-1).double()
        per_face = torch.where(torch.arange(F, device="cuda") % 2 == 0, c * (c + 1) // 2, c * (c - 1) // 2).double()
        pairs = float((per_face * members[block]).sum())
        baked = gm._bake_sums(v, f, T, rgb, R, nb, 1.5)
        d, cs = route()
        same = bool(torch.equal(baked["density"], d) and torch.equal(baked["color_sum"], cs))
        owned = int((torch.from_numpy(tex.texel_owner(F, T)) >= 0).sum())
        del d, cs
        b = timed(lambda: gm.bake_texture(v, f, T, rgb, R, nb), args.warmup, args.runs)
        k = timed(kernel, args.warmup, args.runs)
        r = timed(route, args.warmup, args.runs)
        lines += ["T %4d  cell %d, %d owned texels, %d of %d blocks hold a face (the fullest %d faces), %d slices" % (
                      T, c, owned, int((counts > 0).sum()), nb ** 3, int(counts.max()), slices),
                  "        bake_texture %9.3f [%.3f, %.3f]   gip_texture_bake alone %9.3f [%.3f, %.3f]" % (b + k),
                  "        texel_points + sort by block + gip_field_sample + scatter %9.3f [%.3f, %.3f]   ratio to bake_texture %.2fx" % (
                      r + (r[0] / b[0],)),
                  "        sums bitwise equal to that route: %s" % same,
                  "        %.3e texel-Gaussian evaluations (%.0f per texel), %.1f per ns of gip_texture_bake" % (
                      pairs, pairs / owned, pairs / (k[0] * 1e6))]
    return lines


def decimate(gm, args):
    """clean_mesh, decimate_mesh to 1e5 and 2e4 faces and gip_mesh_cluster_place alone, on the mesh of the default geometry."""
    from gaussianip_amd.utils import mesh
    from gaussianip_amd.utils import texture as tex
    R, nb, T = 128, 16, 4096
    v, f = gm.extract_mesh(resolution=R, num_blocks=nb)
    cv, cf, info = mesh.clean_mesh(v, f, validate=False)
    c = timed(lambda: mesh.clean_mesh(v, f, validate=False), args.warmup, args.runs)
    k = timed(lambda: mesh.connected_components(f, int(v.shape[0])), args.warmup, args.runs)
    lines = ["R %3d  %d vertices, %d faces; atlas cell at T = %d: %d" % (R, v.shape[0], f.shape[0], T, tex.atlas_layout(int(f.shape[0]), T)[0]),
             "       clean_mesh %9.3f [%.3f, %.3f]   connected_components alone %9.3f [%.3f, %.3f]" % (c + k),
             "       %d components, %d kept (min_faces 8, min_diameter 0.05): %d vertices, %d faces; atlas cell %d" % (
                 info["num_components"], info["num_kept"], cv.shape[0], cf.shape[0], tex.atlas_layout(int(cf.shape[0]), T)[0])]
    for target in (100000, 20000):
        dv, df, _, grid = mesh.decimate_mesh(cv, cf, target)
        d = timed(lambda: mesh.decimate_mesh(cv, cf, target), args.warmup, args.runs)
        lines.append("       decimate_mesh to %6d: %9.3f [%.3f, %.3f]   grid %d, %d vertices, %d faces; atlas cell %d" % (
            (target,) + d + (grid, dv.shape[0], df.shape[0], tex.atlas_layout(int(df.shape[0]), T)[0])))
        if grid == 0:
            continue
        one = timed(lambda: mesh.cluster_decimate(cv, cf, grid), args.warmup, args.runs)
        runs = mesh._cluster_runs(cv, cf, grid)
        cells = int(runs["cell_key"].shape[0])
        lines.append("           cluster_decimate at that grid %9.3f [%.3f, %.3f]   %d occupied cells, %.1f corner entries and %.1f vertices per cell" % (
            one + (cells, 3.0 * cf.shape[0] / cells, cv.shape[0] / cells)))
        for lanes in (16, 32, 64):
            p = timed(lambda: mesh._cluster_place(cv, cf, runs, lanes), args.warmup, args.runs)
            lines.append("           gip_mesh_cluster_place alone, %2d lanes per cell %9.3f [%.3f, %.3f]" % ((lanes,) + p))
    return lines


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
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chain-runs", type=int, default=3)
    ap.add_argument("--once", type=int, default=0)
    ap.add_argument("--attributes", action="store_true")
    ap.add_argument("--texture", action="store_true")
    ap.add_argument("--decimate", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "mesh_clean.txt" if args.decimate else "texture_bake.txt" if args.texture else "field_sample.txt" if args.attributes else
                                "field_extract.txt")
    gm = make_model(args.points)
    if args.once:
        gm.extract_mesh(resolution=args.once)
        torch.cuda.synchronize()
        return
    lines = ["tools/bench_field.py: %d Gaussians (human cloud, trained look), %s, median [min, max] of %d runs after %d warm-up, ms" % (
        args.points, "%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName), args.runs, args.warmup)]
    if args.decimate:
        lines += decimate(gm, args)
    elif args.texture:
        lines += texture(gm, args)
    elif args.attributes:
        lines += attributes(gm, args)
    for R in (() if args.attributes or args.texture or args.decimate else (128, 256)):
        field = gm.extract_fields(resolution=R)
        chain, pairs = op_chain(gm, R, count_pairs=True)
        diff = float((field - chain).abs().max() / chain.abs().max())
        v, f = gm.extract_mesh(resolution=R)
        k = timed(lambda: gm.extract_fields(resolution=R), args.warmup, args.runs)
        m = timed(lambda: gm.extract_mesh(resolution=R), args.warmup, args.runs)
        c = timed(lambda: op_chain(gm, R), 1, args.chain_runs)
        lines.append("R %3d  extract_fields %9.3f [%.3f, %.3f]   extract_mesh %9.3f [%.3f, %.3f] (%d vertices, %d faces)" % (
            (R,) + k + m + (v.shape[0], f.shape[0])))
        lines.append("       op chain       %9.3f [%.3f, %.3f] (%d runs)   ratio %.1fx   max |kernel - chain| / max %.2e" % (
            c + (args.chain_runs, c[0] / k[0], diff)))
        lines.append("       %.3e point-Gaussian evaluations, %.1f per ns of extract_fields" % (pairs, pairs / (k[0] * 1e6)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
