#!/usr/bin/env python3
"""Times render_mesh forward + backward with and without what csrc/mesh_grad.hip adds (gradients to vertex positions, the antialias
pass): the blob cloud of tests/sample_inputs.py extracted at resolution 128 with its baked texture, rendered from 4 orbit cameras at
1024 x 1024 as one batch, in three modes:
    off            the keywords off: the gradient of a fixed random upstream gradient to the texture (tools/bench_mesh_render.py's
                   forward_backward)
    positions      position_gradients=True: the same loss, to the texture and the vertices
    positions_aa   position_gradients=True, antialias=True: the same loss plus a fixed random upstream gradient on alpha

Per mode: device events around windows of --iters renders, the median of --windows windows after --warmup windows, per render; then, in
a pass of its own, device events around every call into the library, averaged per entry point (an entry point's own memsets are
inside its figure, torch's allocations and its zeroing of g_pos are not).  With --parent-scene the `off` mode is also timed on the
scene of profiles/mesh_render.json (resolution 256), whose forward_backward figure it should reproduce within that file's spread:
    python tools/bench_mesh_grad.py [--parent-scene] [--out profiles/mesh_grad.json]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench_mesh_render as base  # noqa: E402

SIZE, VIEWS, RESOLUTION = base.SIZE, base.VIEWS, 128
MODES = {"off": dict(), "positions": dict(position_gradients=True), "positions_aa": dict(position_gradients=True, antialias=True)}


def make_scene(resolution):
    base.RESOLUTION = resolution
    return base.make_scene()


def step_of(mode, cams, mesh, g, g_alpha):
    from gaussianip_amd.utils.rasterize import render_mesh
    v, f, _, uv, texture = mesh
    tex = texture.clone().requires_grad_(True)
    verts = v.clone().requires_grad_(bool(MODES[mode]))

    def step():
        tex.grad = verts.grad = None
        out = render_mesh(cams, verts, f, uv, tex, validate=False, **MODES[mode])
        loss = (out["image"] * g).sum()
        if MODES[mode].get("antialias"):
            loss = loss + (out["alpha"] * g_alpha).sum()
        loss.backward()
    return step


def per_entry_point(step, iters):
    """Average device time in microseconds of every gip_mesh_* call of `step`, from events recorded around each call."""
    from gaussianip_amd import _lib
    lib = _lib.model_lib()
    step()                                   # every entry point the step uses is wrapped by now
    saved, events = dict(lib._wrapped), {}
    for name, fn in saved.items():
        if not name.startswith("gip_mesh_"):
            continue

        def timed(*args, _fn=fn, _name=name):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            rc = _fn(*args)
            t1.record()
            events.setdefault(_name, []).append((t0, t1))
            return rc
        lib._wrapped[name] = timed
    try:
        for _ in range(iters):
            step()
        torch.cuda.synchronize()
    finally:
        lib._wrapped.clear()
        lib._wrapped.update(saved)
    return {name: {"calls_per_step": len(ev) / iters, "average_us": 1e3 * sum(a.elapsed_time(b) for a, b in ev) / len(ev)}
            for name, ev in sorted(events.items())}


def measure_scene(args, resolution, modes):
    _, cams, mesh = make_scene(resolution)
    v, f, _, uv, texture = mesh
    gen = torch.Generator(device="cuda").manual_seed(0)
    g = torch.randn((VIEWS, 3, SIZE, SIZE), device="cuda", generator=gen)
    g_alpha = torch.randn((VIEWS, 1, SIZE, SIZE), device="cuda", generator=gen)
    out = {"scene": "blob_cloud extracted at resolution %d, %d orbit cameras at %d x %d as one batch" % (resolution, VIEWS, SIZE, SIZE),
           "counts": {"faces": int(f.shape[0]), "vertices": int(v.shape[0]), "texture_size": int(texture.shape[0])}}
    for mode in modes:
        step = step_of(mode, cams, mesh, g, g_alpha)
        out[mode] = {"forward_backward": base.windows(step, args.iters, args.windows, args.warmup),
                     "entry_points": per_entry_point(step, args.iters)}
    if "positions_aa" in modes:
        from gaussianip_amd.utils.rasterize import render_mesh
        with torch.no_grad():
            r = render_mesh(cams, v, f, uv, texture, validate=False, antialias=True)
        out["counts"]["covered_pixels"] = int((r["rast"][..., 3] > 0).sum())
        out["counts"]["blended_pixels"] = int(((r["alpha"] > 0) & (r["alpha"] < 1)).sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=11)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-scene", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_grad.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mesh_grad needs a GPU"
    result = {"device": "%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName),
              "timing": "device events, median of %d windows of %d renders after %d warm-up windows, ms per forward + backward of the batch; "
                        "entry points: events around every call in a pass of its own, microseconds" % (args.windows, args.iters, args.warmup)}
    result.update(measure_scene(args, RESOLUTION, list(MODES)))
    if args.parent_scene:
        parent = measure_scene(args, 256, ["off"])
        with open(os.path.join(ROOT, "profiles", "mesh_render.json")) as fh:
            recorded = json.load(fh)["forward_backward"]
        result["parent_scene_off"] = dict(parent, recorded_in_mesh_render_json=recorded)
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
