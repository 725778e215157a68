#!/usr/bin/env python3
"""Times forward + backward of the three geometry terms of csrc/mesh_geom.hip together (vertex normals under a fixed random weight, the
Laplacian loss, the normal consistency) on an icosphere of level 8, about 655 thousand vertices and 1.3 million faces, the size of a
resolution-256 extraction, against the same terms spelled with PyTorch operations the way the reference's Mesh spells them:
    hip                 vertex_normals / laplacian_loss / normal_consistency over one MeshTopology built before the clock starts
    torch_as_written    scatter_add of the face normals, edges by sort + unique and the Laplacian's sparse matrix by unique + coalesce
                        rebuilt on every step, as a new reference Mesh per step does
    torch_cached        the same with the edges and the sparse matrix built once, outside the clock: the fair comparison
The modes are timed alternately, window by window, so that they share whatever else the machine is doing: device events around windows
of --iters steps, the median of --windows windows after --warmup windows, milliseconds per step.  Then, in a pass of its own, device
events around every call into the library, averaged per entry point.  The outputs of the two spellings are compared first, at this
size.  MeshTopology's own build time is reported once, by a host clock around a synchronise.
    python tools/bench_mesh_geom.py [--level 8] [--out profiles/mesh_geom.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import mesh_geometry_inputs as inputs  # noqa: E402


def make_mesh(level):
    v, f = inputs.icosphere(level)
    rng = np.random.default_rng(3)
    v = v * inputs.SCALE
    v = v + rng.normal(size=v.shape) * (0.2 * inputs.mean_edge_length(v, f) / 3.0 ** 0.5)
    w = rng.normal(size=v.shape)
    return (torch.from_numpy(v.astype(np.float32)).cuda(), torch.from_numpy(f.astype(np.int32)).cuda(),
            torch.from_numpy(w.astype(np.float32)).cuda())


# ---- the reference's spelling, restated with PyTorch operations
def torch_edges(f):
    e = torch.cat((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]), 0)
    return torch.unique(e.sort(dim=1)[0], dim=0)


def torch_laplacian_matrix(f, V, like):
    ii, jj = f[:, [1, 2, 0]].flatten(), f[:, [2, 0, 1]].flatten()
    adj = torch.stack((torch.cat((ii, jj)), torch.cat((jj, ii))), 0).unique(dim=1)
    ones = torch.ones(adj.shape[1], dtype=like.dtype, device=like.device)
    idx = torch.cat((adj, torch.stack((adj[0], adj[0]), 0)), 1)
    return torch.sparse_coo_tensor(idx, torch.cat((-ones, ones)), (V, V)).coalesce()


def torch_normals(x, f):
    i0, i1, i2 = f[:, 0], f[:, 1], f[:, 2]
    fn = torch.linalg.cross(x[i1] - x[i0], x[i2] - x[i0])
    n = torch.zeros_like(x)
    for i in (i0, i1, i2):
        n = n.scatter_add(0, i[:, None].expand(-1, 3), fn)
    n = torch.where((n * n).sum(-1, keepdim=True) > 1e-20, n, torch.tensor([0.0, 0.0, 1.0], dtype=x.dtype, device=x.device))
    return torch.nn.functional.normalize(n, dim=1)


def torch_terms(x, f, w, edges, L):
    n = torch_normals(x, f)
    en = n[edges]
    nc = (1.0 - torch.cosine_similarity(en[:, 0], en[:, 1], dim=-1)).mean()
    lap = L.mm(x).norm(dim=1).mean()
    return (w * n).sum(), lap, nc


def steps(v, f, w):
    from gaussianip_amd.utils import mesh_geometry as mg
    topo = mg.MeshTopology(f, v.shape[0])
    fl = f.long()
    edges, L = torch_edges(fl), torch_laplacian_matrix(fl, v.shape[0], v)
    x = v.clone().requires_grad_(True)
    out = {}

    def hip():
        x.grad = None
        loss = (w * mg.vertex_normals(x, topo)).sum() + mg.laplacian_loss(x, topo) + mg.normal_consistency(x, topo)
        loss.backward()
        return loss

    def torch_step(cached):
        def step():
            x.grad = None
            with torch.no_grad():
                e, lm = (edges, L) if cached else (torch_edges(fl), torch_laplacian_matrix(fl, v.shape[0], v))
            loss = sum(torch_terms(x, fl, w, e, lm))
            loss.backward()
            return loss
        return step
    out["hip"] = hip
    out["torch_as_written"], out["torch_cached"] = torch_step(False), torch_step(True)
    return out, x, topo


def alternate(fns, iters, count, warmup):
    """{name: windows}: the functions timed in turn, one window each per round."""
    ms = {k: [] for k in fns}
    for r in range(warmup + count):
        for name, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(iters):
                fn()
            t1.record()
            t1.synchronize()
            if r >= warmup:
                ms[name].append(t0.elapsed_time(t1) / iters)
    return {k: {"median_ms": statistics.median(m), "min_ms": min(m), "max_ms": max(m)} for k, m in ms.items()}


def per_entry_point(step, iters):
    """Average device time in microseconds of every gip_mesh_* call of `step`, from events recorded around each call."""
    from gaussianip_amd import _lib
    lib = _lib.model_lib()
    step()
    saved, events = dict(lib._wrapped), {}
    for name, fn in saved.items():
        if not name.startswith("gip_mesh_") or name.endswith("workspace_size"):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=int, default=8)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_geom.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mesh_geom needs a GPU"
    from gaussianip_amd.utils import mesh_geometry as mg
    v, f, w = make_mesh(args.level)
    mg.MeshTopology(f, v.shape[0])             # the first build pays torch's first calls of sort and unique
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    topo = mg.MeshTopology(f, v.shape[0])
    torch.cuda.synchronize()
    build_ms = 1e3 * (time.perf_counter() - t0)
    fns, x, topo = steps(v, f, w)
    result = {"device": "%s (%s)" % (torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName),
              "mesh": "icosphere of level %d scaled by (1.0, 0.8, 1.3) with noise of a fifth of the mean edge length" % args.level,
              "counts": {"vertices": int(v.shape[0]), "faces": int(f.shape[0]), "edges": topo.num_edges, "neighbour_entries": topo.num_neighbours},
              "timing": "device events, modes alternating window by window, median of %d windows of %d steps after %d warm-up windows, ms per "
                        "forward + backward of the three terms; entry points: events around every call in a pass of its own, microseconds; "
                        "topology_build_ms: a host clock around one MeshTopology and a synchronise (the second build of the process)" % (
                            args.windows, args.iters, args.warmup),
              "topology_build_ms": build_ms}
    grads = {}
    for name, fn in fns.items():
        loss = fn()
        grads[name] = (float(loss), x.grad.clone())
    ref = grads["torch_cached"]
    result["agreement_with_torch_cached"] = {
        name: {"loss": val, "gradient_max_abs_difference": float((g - ref[1]).abs().max()), "gradient_max": float(ref[1].abs().max())}
        for name, (val, g) in grads.items()}
    result["forward_backward"] = alternate(fns, args.iters, args.windows, args.warmup)
    result["entry_points"] = per_entry_point(fns["hip"], args.iters)
    text = json.dumps(result, indent=1, sort_keys=True)
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
