#!/usr/bin/env python3
"""Fused SSIM (csrc/ssim.hip through gaussianip_amd.utils.loss.ssim) against the PyTorch op chain (utils.loss.ssim_torch on CUDA
tensors: five grouped 121-tap convolutions on MIOpen, pointwise ops, autograd), forward + backward of `1 - ssim(a, b)`.

Both paths alternate in one process after a warm-up; per shape the median of >= 11 device-event windows of `--iters` forward +
backward pairs each, the launch counts of one pair (torch.profiler), the algorithmic bytes of the fused path
(forward 2 * 4 * NCHW read + 3 * 4 * NCHW derivative planes written, backward 5 * 4 * NCHW read + 4 * NCHW written) and its share
of the HBM roofline (8 TB/s).  Then the stage-3 step (tools/bench_stage3.py's scene: 100k Gaussians, 4 of 32 views at 1024^2,
L1 only, backward, Adam) with lambda_ssim = 0.2 against 0.0, alternating the same way.

    python tools/exp_ssim.py OUT_DIR [--windows 11] [--iters 20] [--no-stage3]

Writes OUT_DIR/exp_ssim.json and prints it."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
HBM_BYTES_PER_S = 8.0e12


def _windows(fns, windows, iters):
    """{name: [ms per call]} — the callables alternate window by window, so drift hits all alike."""
    import torch
    out = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) / iters)
    return out


def _launches(fn):
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name]
    return len(names), sorted(set(names))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out_dir")
    ap.add_argument("--windows", type=int, default=11)
    ap.add_argument("--iters", type=int, default=20, help="forward + backward pairs per timed window")
    ap.add_argument("--no-stage3", action="store_true")
    a = ap.parse_args()
    if a.windows < 11:
        ap.error("--windows must be >= 11")
    import torch
    from gaussianip_amd.utils import loss
    assert torch.cuda.is_available(), "exp_ssim.py measures on the GPU"
    dev = torch.device("cuda")
    res = {"hbm_roofline_bytes_per_s": HBM_BYTES_PER_S, "windows": a.windows, "iters": a.iters, "shapes": {}}
    for shape in ((4, 3, 415, 290), (4, 3, 1024, 1024)):
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.rand(shape, device=dev, generator=g).requires_grad_(True)
        y = (x.detach() + 0.05 * (torch.rand(shape, device=dev, generator=g) - 0.5)).clamp(0, 1)

        def fused():
            x.grad = None
            (1.0 - loss.ssim(x, y)).backward()

        def chain():
            x.grad = None
            (1.0 - loss.ssim_torch(x, y)).backward()

        for _ in range(5):
            fused()
            chain()
        torch.cuda.synchronize()
        fused()
        gf = x.grad.clone()
        chain()
        agree = float((gf - x.grad).abs().max() / x.grad.abs().max())
        w = _windows({"fused": fused, "op_chain": chain}, a.windows, a.iters)
        n = x.numel()
        fwd_bytes, bwd_bytes = (2 + 3) * 4 * n, (5 + 1) * 4 * n
        ms_f, ms_c = statistics.median(w["fused"]), statistics.median(w["op_chain"])
        nf, names_f = _launches(fused)
        nc, _ = _launches(chain)
        res["shapes"]["x".join(map(str, shape))] = {
            "fused_fwd_bwd_ms_median": ms_f, "op_chain_fwd_bwd_ms_median": ms_c, "speedup": ms_c / ms_f,
            "fused_windows_ms": w["fused"], "op_chain_windows_ms": w["op_chain"],
            "fused_launches": nf, "op_chain_launches": nc, "fused_kernels": names_f,
            "fused_algorithmic_bytes": {"forward": fwd_bytes, "backward": bwd_bytes},
            "op_chain_saved_bytes_at_least": 5 * 4 * n,
            "fused_share_of_hbm_roofline": (fwd_bytes + bwd_bytes) / HBM_BYTES_PER_S / (ms_f * 1e-3),
            "grad_max_difference_over_max": agree,
            "note": "ms include the scalar glue of `1 - ssim` (mean, rsub, their backward): the share of the roofline is end to end, "
                    "not a kernel's"}
    if not a.no_stage3:
        import bench_stage3
        from gaussianip_amd.guidance.refine import VIEW_IDX_ALL
        from gaussianip_amd.system import StageThreeStep
        gm, pipe, bg, cams, refined = bench_stage3._setup(100000)
        ids = [0, 9, 17, 30]
        steps = {}
        for lam in (0.0, 0.2):
            st = StageThreeStep(gm, pipe, bg, cams, refined, VIEW_IDX_ALL, lambda_l1=10.0, train_bs=4, lambda_ssim=lam)

            def step(st=st):
                out = st.training_step(id_list=ids)
                gm.optimizer.zero_grad(set_to_none=True)
                out["loss"].backward()
                gm.optimizer.step()
            steps["lambda_ssim_%.1f" % lam] = step
        for _ in range(3):
            for fn in steps.values():
                fn()
        torch.cuda.synchronize()
        w = _windows(steps, a.windows, 5)
        med = {k: statistics.median(v) for k, v in w.items()}
        res["stage3_step"] = {"workload": "100k Gaussians (sh_degree 0), views %s of the 32-view orbit at 1024^2, crop, half size, 10 L1 "
                                          "(+ 0.2 (1 - ssim)), backward, Adam; 5 steps per window" % ids,
                              "ms_per_step_median": med, "ssim_term_ms": med["lambda_ssim_0.2"] - med["lambda_ssim_0.0"], "windows_ms": w}
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, "exp_ssim.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
