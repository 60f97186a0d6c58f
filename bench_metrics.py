#!/usr/bin/env python
"""Evaluation-metrics benchmark (standalone; not the headline metric): freesplat_amd.metrics.image_metrics (fused SSIM +
PSNR, fs_image_metrics) and depth_metrics (fs_depth_metrics) at the evaluation sizes, with the float64 NumPy restatement
of skimage's SSIM (tests/metrics_ref.py -- a restatement, not skimage itself) timed beside them.  Prints one JSON object.

  python bench_metrics.py [--reps 50 --warmup 5 --cpu-views 1]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

SHAPES = [(16, 968, 1296), (8, 384, 512), (16, 480, 640)]   # BASELINE config 3, the native context size, config 2
C = 3
HBM_BYTES_PER_S = 6.29e12      # measured float4 copy rate (MI355X_MICROARCH: HBM3E)
FP32_FLOPS = 157.3e12          # vector fp32 peak
# fp32 operations per kept output pixel and channel, as the kernel forms them: vertical pass 11 taps x (2 mul + 2 add +
# 3 fma x 2), horizontal pass 5 moments x 11 fma x 2, S ~20; plus 5 per pixel for the squared error
FLOPS_PER_OUTPUT = 11 * (2 + 2 + 3 * 2) + 5 * 11 * 2 + 20
FLOPS_PER_PIXEL = 5


def image_bytes(B, H, W):
    return 2 * B * C * H * W * 4


def image_flops(B, H, W):
    return B * C * ((H - 10) * (W - 10) * FLOPS_PER_OUTPUT + H * W * FLOPS_PER_PIXEL)


def gpu_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(3):                       # three windows of `reps` calls; the median window is reported
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / reps)
    return sorted(times)[1], times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-views", type=int, default=1)
    args = ap.parse_args()
    assert args.reps >= 20, "at least 20 repetitions per window"
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py needs a HIP device (no CPU fallback)")
    import metrics_ref as R
    from freesplat_amd import metrics as M
    dev = torch.device("cuda:0")
    out = {"bench": "metrics", "C": C, "shapes": []}
    for B, H, W in SHAPES:
        g = torch.Generator(device=dev).manual_seed(B * H + W)
        gt = torch.rand(B, C, H, W, device=dev, generator=g)
        pred = (gt + 0.05 * torch.randn(B, C, H, W, device=dev, generator=g)).clamp(0, 1)
        ms, windows = gpu_ms(lambda: M.image_metrics(gt, pred), args.reps, args.warmup)
        nbytes, flops = image_bytes(B, H, W), image_flops(B, H, W)
        t_mem, t_alu = nbytes / HBM_BYTES_PER_S, flops / FP32_FLOPS
        bound = "hbm" if t_mem >= t_alu else "fp32_vector"
        dgt = torch.rand(B, H, W, device=dev, generator=g) * 5
        dpred = dgt * (1 + 0.2 * (torch.rand(B, H, W, device=dev, generator=g) - 0.5))
        dms, _ = gpu_ms(lambda: M.depth_metrics(dgt, dpred), args.reps, args.warmup)
        # CPU restatement on the first views, and parity of view 0
        g_np, p_np = gt[:args.cpu_views].cpu().numpy(), pred[:args.cpu_views].cpu().numpy()
        t0 = time.perf_counter()
        ref = [R.ssim(a, b) for a, b in zip(g_np, p_np)]
        cpu_s = (time.perf_counter() - t0) / args.cpu_views
        ssim = M.image_metrics(gt, pred)[1]
        row = {
            "B": B, "H": H, "W": W,
            "image_metrics_ms_per_call": round(ms, 4), "image_metrics_windows_ms": [round(t, 4) for t in windows],
            "us_per_view": round(1e3 * ms / B, 2),
            "algorithmic_bytes": nbytes, "fp32_ops": flops,
            "hbm_floor_us": round(1e6 * t_mem, 2), "fp32_floor_us": round(1e6 * t_alu, 2), "bound": bound,
            "share_of_hbm_peak": round(1e3 * t_mem / ms, 3), "share_of_fp32_peak": round(1e3 * t_alu / ms, 3),
            "depth_metrics_ms_per_call": round(dms, 4),
            "cpu_baseline": {"what": "float64 NumPy restatement of skimage SSIM (tests/metrics_ref.py), not skimage",
                             "views": args.cpu_views, "s_per_view": round(cpu_s, 4)},
            "parity": {"max_abs_ssim_diff_view0": float(abs(float(ssim[0]) - ref[0]))},
        }
        out["shapes"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
