#!/usr/bin/env python3
"""Measures the chart atlas of gaussianip_amd/utils/uv_atlas.py (csrc/mesh_uv.hip) and writes profiles/uv_atlas.json.

Unwrapping, on the project's own extracted meshes (the 100k-Gaussian human cloud of tests/scenes.py with the trained look, extract_mesh
at resolution 128 and 256, the meshes DESIGN.md quotes): for smooth_rounds in 0, 2, 4, 8 the number of charts, the share of charts
under 8 faces, the atlas' occupancy (texels the UV triangles cover over T^2, from ChartAtlas.texel_points), the scale found and the
time of one unwrap_charts by a host clock around a synchronise (the median of --runs runs after one warm-up: the call reads back
the label rounds' flag, the charts' boxes and the faces' areas, so a host clock is the honest one).

Tangents, on the level-8 icosphere of tools/bench_mesh_geom.py (655k vertices): forward + backward of vertex_tangents under a fixed
random weight against the same formula (the reference's Mesh._compute_vertex_tangent) spelled with PyTorch operations, the per-vertex
sums as scatter_add of the face tangents, with the same atlas; device events, modes alternating window by window, the median of --windows
windows of --iters steps.  The two spellings' outputs are compared first.
    python tools/bench_uv_atlas.py [--out profiles/uv_atlas.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_field  # noqa: E402
import bench_mesh_geom  # noqa: E402


def unwrap_figures(v, f, T, rounds_list, runs):
    from gaussianip_amd.utils.uv_atlas import unwrap_charts
    out = {}
    for rounds in rounds_list:
        atlas = unwrap_charts(v, f, T, smooth_rounds=rounds)      # warm-up, and the atlas the figures are read from
        times = []
        for _ in range(runs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            unwrap_charts(v, f, T, smooth_rounds=rounds)
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
        faces_per_chart = torch.bincount(atlas.face_chart.long(), minlength=atlas.num_charts)
        covered, _, _ = atlas.texel_points(v)
        out[str(rounds)] = {"charts": atlas.num_charts, "charts_under_8_faces": int((faces_per_chart < 8).sum()),
                            "share_of_charts_under_8_faces": float((faces_per_chart < 8).float().mean()),
                            "faces_in_charts_under_8_faces": int(faces_per_chart[faces_per_chart < 8].sum()),
                            "texture_vertices": int(atlas.v_tex.shape[0]), "texels_per_unit": atlas.scale,
                            "occupancy": float(covered.float().mean()), "unwrap_ms_median": statistics.median(times),
                            "unwrap_ms_min": min(times), "unwrap_ms_max": max(times)}
        print("F %d T %d rounds %d: %s" % (f.shape[0], T, rounds, out[str(rounds)]), flush=True)
    return out


def torch_tangents(x, n, f, v_tex, t_idx):
    """The tangent formula of csrc/mesh_uv.hip's header with PyTorch operations, the per-vertex sums as scatter_add."""
    p, t = x[f], v_tex[t_idx]                                              # [F, 3, 3], [F, 3, 2]
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    a, b = t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]
    den = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    den = torch.where(den > 0, den.clamp(min=1e-6), den.clamp(max=-1e-6))
    face = (e1 * b[:, 1:2] - e2 * a[:, 1:2]) / den[:, None]
    rows = f.reshape(-1, 1).expand(-1, 3)
    total = torch.zeros_like(n).scatter_add(0, rows, face.repeat_interleave(3, 0))
    count = torch.zeros_like(n).scatter_add(0, rows, torch.ones_like(rows, dtype=n.dtype))
    t1 = torch.nn.functional.normalize(total / count, dim=1)
    return torch.nn.functional.normalize(t1 - (t1 * n).sum(1, keepdim=True) * n, dim=1)


def tangent_figures(level, windows, iters, warmup):
    from gaussianip_amd.utils import mesh_geometry as mg
    from gaussianip_amd.utils.uv_atlas import unwrap_charts, vertex_tangents
    v, f, w = bench_mesh_geom.make_mesh(level)
    topo = mg.MeshTopology(f, v.shape[0])
    atlas = unwrap_charts(v, f, 8192)
    nrm = mg.vertex_normals(v, topo).detach()
    x = v.clone().requires_grad_(True)
    n = nrm.clone().requires_grad_(True)
    fl, tl = f.long(), atlas.t_tex_idx.long()

    def hip():
        x.grad = n.grad = None
        loss = (w * vertex_tangents(x, topo, atlas.v_tex, atlas.t_tex_idx, n)).sum()
        loss.backward()
        return loss

    def torch_ops():
        x.grad = n.grad = None
        loss = (w * torch_tangents(x, n, fl, atlas.v_tex, tl)).sum()
        loss.backward()
        return loss
    grads = {}
    for name, fn in (("hip", hip), ("torch_ops", torch_ops)):
        loss = fn()
        grads[name] = (float(loss), x.grad.clone(), n.grad.clone())
    ref = grads["torch_ops"]
    agreement = {"loss_hip": grads["hip"][0], "loss_torch_ops": ref[0],
                 "g_vertices_max_abs_difference": float((grads["hip"][1] - ref[1]).abs().max()), "g_vertices_max": float(ref[1].abs().max()),
                 "g_normals_max_abs_difference": float((grads["hip"][2] - ref[2]).abs().max()), "g_normals_max": float(ref[2].abs().max())}
    timing = bench_mesh_geom.alternate({"hip": hip, "torch_ops": torch_ops}, iters, windows, warmup)
    return {"counts": {"vertices": int(v.shape[0]), "faces": int(f.shape[0]), "texture_vertices": int(atlas.v_tex.shape[0]),
                       "charts": atlas.num_charts}, "agreement": agreement, "forward_backward": timing}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaussians", type=int, default=100000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--level", type=int, default=8)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "uv_atlas.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_uv_atlas needs a GPU"
    result = {"device": "%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName),
              "timing": "unwrap: a host clock around one unwrap_charts and a synchronise, median of %d runs after a warm-up, ms; tangents: "
                        "device events, modes alternating window by window, median of %d windows of %d steps after %d warm-up windows, "
                        "ms per forward + backward" % (args.runs, args.windows, args.iters, args.warmup),
              "unwrap": {}}
    gm = bench_field.make_model(args.gaussians)
    for resolution, T in ((128, 4096), (256, 8192)):
        v, f = gm.extract_mesh(density_thresh=1.0, resolution=resolution, num_blocks=16)
        key = "R%d_F%d_T%d" % (resolution, f.shape[0], T)
        result["unwrap"][key] = unwrap_figures(v, f, T, (0, 2, 4, 8), args.runs)
    result["tangents"] = tangent_figures(args.level, args.windows, args.iters, args.warmup)
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
