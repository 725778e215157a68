#!/usr/bin/env python3
"""Cost of the antialiasing mode (GaussianRasterizationSettings.antialiasing) on the BASELINE configs[1] workload: 100k Gaussians
(human init, sh_degree 0), the 4-view launch set at 1024^2, forward + backward.  Flag off and on alternate in one process after a
warm-up; reports the median of >= 11 device-event windows of forward + backward per flag, the per-stage times of
rasterizer.profile_stages, and num_rendered in the default list mode (and the trained look's num_rendered).

    python tools/exp_antialiasing.py OUT_DIR [--windows 11] [--iters 10]

Writes OUT_DIR/exp_antialiasing.json and prints it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--windows", type=int, default=11)
    ap.add_argument("--iters", type=int, default=10, help="forward + backward pairs per timed window")
    a = ap.parse_args()
    if a.windows < 11:
        ap.error("--windows must be >= 11")
    import torch
    import scenes
    from gaussianip_amd import GaussianRasterizationSettings, rasterize_views
    from gaussianip_amd import rasterizer as R
    dev = torch.device("cuda")
    P, V, H, W = 100000, 4, 1024, 1024
    cams = scenes.train_cameras(V, 42, H, W)
    bg = torch.zeros(3, device=dev)

    def settings(aa):
        return [GaussianRasterizationSettings(
            image_height=H, image_width=W, tanfovx=c["tanfovx"], tanfovy=c["tanfovy"], bg=bg, scale_modifier=1.0,
            viewmatrix=torch.from_numpy(c["viewmatrix"]).to(dev), projmatrix=torch.from_numpy(c["projmatrix"]).to(dev),
            sh_degree=0, campos=torch.from_numpy(c["campos"]).to(dev), prefiltered=False, debug=False, antialiasing=aa) for c in cams]

    sts = {False: settings(False), True: settings(True)}
    looks = {"init": scenes.make_scene("human", P, seed=42), "trained": scenes.trained_look(scenes.make_scene("human", P, seed=42), seed=7)}
    g = torch.Generator(device=dev).manual_seed(0)
    gC = torch.randn((V, 3, H, W), device=dev, generator=g)
    gD = torch.randn((V, 1, H, W), device=dev, generator=g)
    res = dict(workload="BASELINE configs[1]: P=%d, V=%d, %dx%d, sh_degree 0, default list mode" % (P, V, H, W))

    for look, sc in looks.items():
        t = {k: torch.from_numpy(v).to(dev).requires_grad_(True) for k, v in sc.items()}

        def step(aa):
            color, radii, depth, alpha = rasterize_views(t["means3D"], None, t["opacities"], sts[aa], shs=t["shs"],
                                                         scales=t["scales"], rotations=t["rotations"])
            torch.autograd.backward([color, depth], [gC, gD])

        entry = {}
        for aa in (False, True):
            with torch.no_grad():
                _, plan = R.forward_with_state(t["means3D"].detach(), t["opacities"].detach(), sts[aa], shs=t["shs"].detach(),
                                               scales=t["scales"].detach(), rotations=t["rotations"].detach())
            entry["num_rendered_" + ("on" if aa else "off")] = int(plan.num_rendered)
        if look == "init":
            for _ in range(3):                                     # warm-up: capacity hints, code objects, caches
                for aa in (False, True):
                    step(aa)
            torch.cuda.synchronize()
            windows = {False: [], True: []}
            for _ in range(a.windows):
                for aa in (False, True):                           # alternate: drift hits both alike
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        step(aa)
                    e1.record()
                    e1.synchronize()
                    windows[aa].append(e0.elapsed_time(e1) / a.iters)
            for aa in (False, True):
                k = "on" if aa else "off"
                entry["fwd_bwd_ms_median_" + k] = statistics.median(windows[aa])
                entry["fwd_bwd_ms_windows_" + k] = windows[aa]
            stages = {False: [], True: []}
            for _ in range(3):
                for aa in (False, True):
                    ms, _ = R.profile_stages(t["means3D"].detach(), t["opacities"].detach(), sts[aa], gC, g_depth=gD,
                                             shs=t["shs"].detach(), scales=t["scales"].detach(), rotations=t["rotations"].detach(),
                                             iters=a.iters)
                    stages[aa].append(ms)
            for aa in (False, True):
                entry["stages_ms_" + ("on" if aa else "off")] = {n: statistics.median(s[n] for s in stages[aa]) for n in R.STAGE_NAMES}
        res[look] = entry
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "exp_antialiasing.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
