#!/usr/bin/env python3
"""Times the mesh renderer (csrc/mesh_raster.hip, gaussianip_amd/utils/rasterize.py): the blob cloud of tests/sample_inputs.py extracted
at resolution 256 with its baked texture, rendered from 4 orbit cameras at 1024 x 1024 as one batch, forward and forward + backward
(the gradient of a fixed random upstream gradient to the texture).

Times are device events around windows of --iters renders: the median of --windows windows after --warmup windows, per render.
Kernel times come from a kernel trace taken in a run of its own and are merged afterwards:
    python tools/bench_mesh_render.py [--out profiles/mesh_render.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_mesh_render.py --once 20
    python tools/bench_mesh_render.py --kernel-stats DIR/*/*_kernel_stats.csv [--out profiles/mesh_render.json]
Beside every kernel's time stand the bytes it must move (computed here from the shapes and the counts of the scene, not measured)
and the share of the HBM roofline that makes: those bytes over the time, over 8.0 TB/s (the float atomic adds of the backward over the
1.3 TB/s at which the chip adds).

--mip times the pieces of MipMeshRasterizerContext (csrc/mesh_mip.hip) on the same scene, each entry point on its own with device
events: gip_mesh_rast_db, the build of the mip stack of a 4096 x 4096 x 3 texture, gip_mesh_texture_mip forward and backward (the
backward with its fold), and beside them the bilinear gip_mesh_texture forward and backward at the same uv as the yardstick.  The uv
are per vertex (its x, y inside the mesh's bounding box), interpolated per pixel with their differentials:
    python tools/bench_mesh_render.py --mip [--out profiles/mesh_mip.json]

--texture-project times the bake of the texture from rendered views (csrc/texture_project.hip, GaussianModel.bake_texture_from_views) on
the same cloud extracted at resolution 128, with 8 and with 32 orbit cameras at 1024 x 1024: render_views, visible_depth, the packing
of the images and the view table, gip_texture_project itself (with the bytes it must move, from the shapes), and the field bake
(GaussianModel.bake_texture) beside them:
    python tools/bench_mesh_render.py --texture-project --iters 2 [--out profiles/texture_project.json]"""
import argparse
import csv
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12            # bytes per second, the specified peak
ATOMIC_RATE = 1.3e12         # added bytes per second of float atomic adds, chip-wide
SIZE, VIEWS, RESOLUTION = 1024, 4, 256
KERNELS = ("mesh_setup_kernel", "mesh_large_kernel", "mesh_resolve_kernel", "mesh_shade_kernel", "mesh_shade_backward_kernel")


def make_scene():
    import sample_inputs
    import scenes
    from gaussianip_amd.scene import Camera, GaussianModel
    from gaussianip_amd.utils.sh import C0
    cl = sample_inputs.blob_cloud()
    P = cl["xyz"].shape[0]
    gm = GaussianModel(0)
    gm._xyz, gm._opacity = torch.from_numpy(cl["xyz"]).cuda(), torch.from_numpy(cl["opacity"]).cuda()
    gm._scaling, gm._rotation = torch.from_numpy(cl["scaling"]).cuda(), torch.from_numpy(cl["rotation"]).cuda()
    gm._features_dc = ((torch.from_numpy(sample_inputs.colors(P, 9)).cuda() - 0.5) / C0).reshape(P, 1, 3).contiguous()
    gm._features_rest = torch.zeros((P, 0, 3), device="cuda")
    cams = [Camera(c2w=scenes.orbit_c2w(15.0, -180.0 + 90.0 * i, 1.6).cuda(), FoVy=math.radians(50.0), height=SIZE, width=SIZE)
            for i in range(VIEWS)]
    mesh = gm.extract_textured_mesh(density_thresh=1.0, resolution=RESOLUTION, num_blocks=16)
    return gm, cams, mesh


def windows(fn, iters, count, warmup):
    for _ in range(warmup):
        for _ in range(iters):
            fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(count):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1) / iters)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def required_bytes(counts):
    """The bytes every kernel must move at least, from the shapes: name -> (bytes, what they are)."""
    px, F, V, T = counts["pixels"], counts["faces"], counts["vertices"], counts["texture_size"]
    covered, frags = counts["covered_pixels"], counts["fragments_at_least"]
    return {
        "mesh_setup_kernel": (VIEWS * (F * 12 + V * 16) + frags * 8,
                              "per view the index triples and every vertex once, an 8-byte atomic minimum per fragment (at least one per covered pixel)"),
        "mesh_large_kernel": (4, "the list's count; this scene lists no triangle"),
        "mesh_resolve_kernel": (px * 24 + covered * 0, "8-byte key in, 16-byte rast out per pixel (the winning triangle's vertices come from cache)"),
        "mesh_shade_kernel": (px * 32 + counts["visible_faces"] * 24, "16-byte rast in, 16 bytes out per pixel, the visible faces' uv once (texels come from cache)"),
        "mesh_shade_backward_kernel": (px * 32 + counts["visible_faces"] * 24 + covered * 48,
                                       "rast and the upstream gradient in, 12 float atomic adds per covered pixel; its memset of the %d x %d x 3 "
                                       "gradient (%d bytes) is a launch of its own" % (T, T, T * T * 12)),
    }


def measure(args):
    from gaussianip_amd.arguments import PipelineParams
    from gaussianip_amd.renderer import render
    from gaussianip_amd.utils.rasterize import render_mesh
    gm, cams, (v, f, _, uv, texture) = make_scene()
    tex = texture.clone().requires_grad_(True)
    g = torch.randn((VIEWS, 3, SIZE, SIZE), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))

    def forward():
        with torch.no_grad():
            return render_mesh(cams, v, f, uv, texture, validate=False)

    def both():
        tex.grad = None
        (render_mesh(cams, v, f, uv, tex, validate=False)["image"] * g).sum().backward()

    out = forward()
    ids = out["rast"][..., 3].long() - 1
    covered = int((ids >= 0).sum())
    visible = sum(int(torch.unique(ids[b][ids[b] >= 0]).numel()) for b in range(VIEWS))
    counts = {"faces": int(f.shape[0]), "vertices": int(v.shape[0]), "texture_size": int(texture.shape[0]), "views": VIEWS, "image": SIZE,
              "pixels": VIEWS * SIZE * SIZE, "covered_pixels": covered, "visible_faces": visible, "fragments_at_least": covered}
    with torch.no_grad():
        bg = torch.zeros(3, device="cuda")
        gauss = render(cams[0], gm, PipelineParams(argparse.ArgumentParser()), bg)["render"]
        psnr = -10 * math.log10(float(((gauss - out["image"][0]) ** 2).mean()))
    result = {"device": "%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName),
              "scene": "blob_cloud extracted at resolution %d, %d orbit cameras at %d x %d as one batch" % (RESOLUTION, VIEWS, SIZE, SIZE),
              "counts": counts, "psnr_db_mesh_vs_gaussians_view0": psnr,
              "timing": "device events, median of %d windows of %d renders after %d warm-up windows, ms per render of the batch" % (
                  args.windows, args.iters, args.warmup),
              "forward": windows(forward, args.iters, args.windows, args.warmup),
              "forward_backward": windows(both, args.iters, args.windows, args.warmup)}
    return result


MIP_TEXTURE = 4096


def measure_mip(args):
    """Every piece as one call through the context, timed alone.  The texture is random (the lookup's cost does not depend on its
    values).  The baked atlas has no continuous layout, so the uv here are per vertex: its x and y inside the mesh's bounding box,
    which spreads 4096 texels over the few hundred pixels the mesh covers, at a density that changes with the surface's angle."""
    from gaussianip_amd.utils.rasterize import MipMeshRasterizerContext
    _, cams, (v, f, _, uv, texture) = make_scene()
    ctx = MipMeshRasterizerContext()
    gen = torch.Generator(device="cuda").manual_seed(0)
    mvp = torch.stack([c.full_proj_transform.float() for c in cams])
    pos = torch.matmul(torch.cat((v, torch.ones_like(v[:, :1])), 1)[None], mvp).contiguous()
    rast, rast_db = ctx.rasterize(pos, f, SIZE, validate=False)
    # per-vertex texture coordinates with a continuous layout: the vertex's position in its bounding box, x and y
    lo, hi = v.min(0).values, v.max(0).values
    attr = ((v - lo) / (hi - lo))[:, :2].contiguous()
    st, st_da = ctx.interpolate(attr, rast, f, rast_db=rast_db, diff_attrs="all")
    # An empty pixel interpolates to uv (0, 0): left there, the 2.4 M empty pixels of this scene would all add their gradient to the one
    # texel (0, 0), and the backward would time that contention (362 ms, against 1 ms without it) and not the lookup.  They look up a
    # screen-aligned background instead: their own position, 4 texels a pixel.
    empty = (rast[..., 3:] == 0)
    ramp = (torch.arange(SIZE, device="cuda", dtype=torch.float32) + 0.5) / SIZE
    screen = torch.stack(torch.meshgrid(ramp, ramp, indexing="xy"), -1)[None].expand(VIEWS, SIZE, SIZE, 2)
    st = torch.where(empty, screen, st).contiguous()
    st_da = torch.where(empty, torch.tensor([1.0 / SIZE, 0.0, 0.0, 1.0 / SIZE], device="cuda"), st_da).contiguous()
    tex = torch.rand((MIP_TEXTURE, MIP_TEXTURE, 3), device="cuda", generator=gen)
    g = torch.randn((VIEWS, SIZE, SIZE, 3), device="cuda", generator=gen)
    stack = ctx.texture_construct_mip(tex)
    covered = rast[..., 3] > 0
    with torch.no_grad():
        sx, sy, tx, ty = (st_da[..., k] * MIP_TEXTURE for k in range(4))
        A, B, C = sx * sx + tx * tx, sy * sy + ty * ty, sx * sy + tx * ty
        level = 0.5 * torch.log2(0.5 * (A + B) + torch.sqrt(0.25 * (A - B) ** 2 + C * C))[covered]
        lc = level.clamp(0, stack.L)
    tex_g, st_g = tex.clone().requires_grad_(True), st.clone().requires_grad_(True)
    da_g = st_da.clone().requires_grad_(True)

    def backward_of(fn):
        def run():
            tex_g.grad = st_g.grad = da_g.grad = None
            fn().backward(g)
        return run

    timed = {
        "gip_mesh_rast_db": lambda: ctx.rasterize(pos, f, SIZE, validate=False),
        "gip_mesh_rasterize_alone": lambda: super(MipMeshRasterizerContext, ctx).rasterize(pos, f, SIZE, validate=False),
        "mip_build_4096": lambda: ctx.texture_construct_mip(tex),
        "gip_mesh_texture_mip_forward": lambda: ctx.texture(tex, st, uv_da=st_da, mip=stack),
        "gip_mesh_texture_mip_forward_backward": backward_of(lambda: ctx.texture(tex_g, st_g, uv_da=da_g, mip=stack)),
        "gip_mesh_texture_forward": lambda: ctx.texture(tex, st),
        "gip_mesh_texture_forward_backward": backward_of(lambda: ctx.texture(tex_g, st_g)),
    }
    with torch.no_grad():
        times = {k: windows(fn, args.iters, args.windows, args.warmup) for k, fn in timed.items() if "backward" not in k}
    times.update({k: windows(fn, args.iters, args.windows, args.warmup) for k, fn in timed.items() if "backward" in k})
    med = lambda k: times[k]["median_ms"]  # noqa: E731
    derived = {
        "rast_db_ms": med("gip_mesh_rast_db") - med("gip_mesh_rasterize_alone"),
        "texture_mip_backward_ms": med("gip_mesh_texture_mip_forward_backward") - med("gip_mesh_texture_mip_forward"),
        "texture_backward_ms": med("gip_mesh_texture_forward_backward") - med("gip_mesh_texture_forward"),
        "forward_ratio_to_bilinear": med("gip_mesh_texture_mip_forward") / med("gip_mesh_texture_forward"),
        "forward_backward_ratio_to_bilinear": med("gip_mesh_texture_mip_forward_backward") / med("gip_mesh_texture_forward_backward"),
    }
    return {"device": "%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName),
            "scene": "blob_cloud extracted at resolution %d, %d orbit cameras at %d x %d as one batch, a random %d x %d x 3 texture looked up "
                     "at per-vertex uv (the vertex's x, y in the mesh's bounding box) with their pixel differentials; empty pixels look up their screen position, 4 texels a pixel" % (
                         RESOLUTION, VIEWS, SIZE, SIZE, MIP_TEXTURE, MIP_TEXTURE),
            "counts": {"pixels": VIEWS * SIZE * SIZE, "covered_pixels": int(covered.sum()), "faces": int(f.shape[0]), "levels": stack.L,
                       "level_of_detail_quartiles_covered": [float(x) for x in torch.quantile(level.float(), torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0], device="cuda"))],
                       "share_of_covered_pixels_reading_two_levels": float(((lc > 0) & (lc < stack.L)).float().mean())},
            "timing": "device events, median of %d windows of %d calls after %d warm-up windows, ms per call through the Python context; "
                      "the backward rows are forward + backward, the derived rows their difference; rast_db_ms is rasterize with rast_db "
                      "minus rasterize alone; the mip backward includes both memsets and the fold" % (args.windows, args.iters, args.warmup),
            "times": times, "derived": derived}


PROJECT_RESOLUTION, PROJECT_VIEWS = 128, (8, 32)


def measure_texture_project(args):
    import ctypes

    import sample_inputs
    import scenes
    from gaussianip_amd import _lib
    from gaussianip_amd.arguments import PipelineParams
    from gaussianip_amd.renderer import render_views
    from gaussianip_amd.scene import Camera, GaussianModel
    from gaussianip_amd.utils import texture as tex
    from gaussianip_amd.utils.sh import C0
    cl = sample_inputs.blob_cloud()
    P = cl["xyz"].shape[0]
    gm = GaussianModel(0)
    gm._xyz, gm._opacity = torch.from_numpy(cl["xyz"]).cuda(), torch.from_numpy(cl["opacity"]).cuda()
    gm._scaling, gm._rotation = torch.from_numpy(cl["scaling"]).cuda(), torch.from_numpy(cl["rotation"]).cuda()
    gm._features_dc = ((torch.from_numpy(sample_inputs.colors(P, 9)).cuda() - 0.5) / C0).reshape(P, 1, 3).contiguous()
    gm._features_rest = torch.zeros((P, 0, 3), device="cuda")
    pipe, bg = PipelineParams(argparse.ArgumentParser()), torch.zeros(3, device="cuda")
    kw = dict(resolution=PROJECT_RESOLUTION, num_blocks=16)
    with torch.no_grad():
        v, f = gm.extract_mesh(density_thresh=1.0, **kw)
    F, V = int(f.shape[0]), int(v.shape[0])
    T = gm._default_texture_size(F)
    c = tex.atlas_layout(F, T)[0]
    owned = int((tex.texel_owner(F, T) >= 0).sum())
    tol = 2.0 / (PROJECT_RESOLUTION - 1) / float(gm.scale)
    result = {"device": "%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName),
              "scene": "blob_cloud extracted at resolution %d: %d faces, texture %d (cell %d, %d owned texels); orbit cameras at %d x %d" % (
                  PROJECT_RESOLUTION, F, T, c, owned, SIZE, SIZE),
              "timing": "device events, median of %d windows of %d calls after %d warm-up windows, ms per call" % (args.windows, args.iters, args.warmup),
              "field_bake": windows(lambda: gm.bake_texture(v, f, T, **kw), args.iters, args.windows, args.warmup)}
    lib = _lib.model_lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for K in PROJECT_VIEWS:
        cams = [Camera(c2w=scenes.orbit_c2w(15.0 if i % 2 else -15.0, -180.0 + 360.0 * i / K, 1.6).cuda(), FoVy=math.radians(50.0), height=SIZE,
                       width=SIZE) for i in range(K)]

        def render_all():
            with torch.no_grad():
                pkgs = [render_views(cams[i:i + _lib.GIP_MAX_VIEWS], gm, pipe, bg) for i in range(0, K, _lib.GIP_MAX_VIEWS)]
            return torch.cat([q["render"] for q in pkgs]).detach(), torch.cat([q["alpha_3dgs"] for q in pkgs]).detach()
        images, alphas = render_all()
        vis = tex.visible_depth(cams, v, f, validate=False)

        def pack():
            return torch.cat((images, alphas), 1).permute(0, 2, 3, 1).contiguous(), tex.pack_views(cams, v.device)
        packed, table = pack()
        sums = [torch.zeros((T, T, 3), device="cuda"), torch.zeros((T, T), device="cuda"), torch.zeros((T, T), dtype=torch.int32, device="cuda")]
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def kernel():
            rc = lib.gip_texture_project(p(v), V, p(f), F, T, c, K, p(table), p(packed), p(vis), SIZE, SIZE, tol, 0.2, 0.5, 1, 1, p(sums[0]), p(sums[1]),
                                         p(sums[2]), stream)
            assert rc == 0, rc
        kernel()
        covered = int((vis > 0).sum())
        need = owned * 20 + F * 12 + V * 12 + K * 80 + covered * 20
        entry = {"render_views": windows(render_all, args.iters, args.windows, args.warmup),
                 "visible_depth": windows(lambda: tex.visible_depth(cams, v, f, validate=False), args.iters, args.windows, args.warmup),
                 "pack": windows(pack, args.iters, args.windows, args.warmup),
                 "gip_texture_project": windows(kernel, args.iters, args.windows, args.warmup),
                 "bake_texture_from_views": windows(lambda: gm.bake_texture_from_views(v, f, cams, pipe, T, **kw), args.iters, args.windows, args.warmup),
                 "texels_seen": int((sums[2] > 0).sum()), "texels_owned": owned, "covered_pixels": covered,
                 "kernel_required_bytes": need,
                 "kernel_required_bytes_note": "20 bytes written per owned texel, the faces and vertices once, the view table, and 20 bytes "
                                               "(one 16-byte tap and one depth) per covered pixel of every view; neighbouring taps come from cache"}
        entry["kernel_share_of_hbm_peak"] = need / (entry["gip_texture_project"]["median_ms"] * 1e-3) / HBM_PEAK
        result["views_%d" % K] = entry
    return result


def merge_kernel_stats(result, path):
    """Per-kernel average times of a `rocprofv3 --kernel-trace --stats` run of `--once`, with the bytes each kernel must move."""
    need = required_bytes(result["counts"])
    kernels = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name", "")
            for k in KERNELS:
                if name.startswith(k):
                    avg_ns = float(row["AverageNs"])
                    nbytes, what = need[k]
                    atomics = result["counts"]["covered_pixels"] * 48 if k == "mesh_shade_backward_kernel" else 0
                    floor_s = max(nbytes / HBM_PEAK, atomics / ATOMIC_RATE)
                    kernels[k] = {"calls": int(row["Calls"]), "average_us": avg_ns / 1e3, "min_us": float(row["MinNs"]) / 1e3,
                                  "max_us": float(row["MaxNs"]) / 1e3, "required_bytes": nbytes, "required_bytes_are": what,
                                  "achieved_TB_per_s": nbytes / avg_ns / 1e3, "hbm_roofline_fraction": nbytes / HBM_PEAK / (avg_ns * 1e-9),
                                  "bound_fraction_with_atomic_rate": floor_s / (avg_ns * 1e-9)}
    result["kernels"] = kernels
    result["kernel_times_from"] = "rocprofv3 --kernel-trace --stats of --once, a run of its own"
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=11)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--once", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--mip", action="store_true", help="time the pieces of MipMeshRasterizerContext instead")
    ap.add_argument("--texture-project", action="store_true", help="time the bake of the texture from rendered views instead")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "texture_project.json" if args.texture_project else "mesh_mip.json" if args.mip else "mesh_render.json")
    if args.texture_project:
        assert torch.cuda.is_available(), "bench_mesh_render needs a GPU"
        result = measure_texture_project(args)
    elif args.mip:
        assert torch.cuda.is_available(), "bench_mesh_render needs a GPU"
        result = measure_mip(args)
    elif args.kernel_stats:
        with open(args.out) as fh:
            result = json.load(fh)
        result = merge_kernel_stats(result, args.kernel_stats)
    elif args.once:
        from gaussianip_amd.utils.rasterize import render_mesh
        _, cams, (v, f, _, uv, texture) = make_scene()
        tex = texture.clone().requires_grad_(True)
        g = torch.randn((VIEWS, 3, SIZE, SIZE), device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
        for _ in range(args.once):
            tex.grad = None
            (render_mesh(cams, v, f, uv, tex, validate=False)["image"] * g).sum().backward()
        torch.cuda.synchronize()
        return
    else:
        assert torch.cuda.is_available(), "bench_mesh_render needs a GPU"
        result = measure(args)
        if os.path.exists(args.out):      # what tests/test_gpu_mesh_render.py added to the file stays
            with open(args.out) as fh:
                kept = json.load(fh).get("alignment_test_128")
            if kept is not None:
                result["alignment_test_128"] = kept
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
