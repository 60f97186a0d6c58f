#!/usr/bin/env python
"""SSIM / photometric-loss benchmark (standalone; not the headline metric).  One process, every shape warmed first.

  fused    freesplat_amd.ssim_loss.photometric_loss (fs_ssim_loss_forward / _backward), forward under no_grad and
           forward + backward to the prediction
  eager    the same loss as a user writes it today: tests/ssim_loss_ref.py in float32 on the same device (five grouped
           separable conv2d pairs under autograd) -- a yardstick, not code under test
for 4 views x 3 x 968 x 1296 (config 3's targets) and 8 x 3 x 384 x 512, both conventions.  Fused and eager windows alternate
inside one session; the median window and the spread (min, max) of the per-call times are reported, with the bytes each form
holds between forward and backward (torch.cuda.memory_allocated after the forward minus before it), the algorithmic bytes and
fp32 operations of the fused kernels and their share of the HBM and vector-fp32 peaks.

Prints one JSON object and writes it to --out.    python bench_ssim_loss.py [--reps 7 --warmup 3 --out profiles/ssim_loss_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch

SIZES = [(4, 3, 968, 1296), (8, 3, 384, 512)]
HBM_BYTES_PER_S = 6.29e12          # measured streaming rate and vector-fp32 peak used by DESIGN.md "Evaluation metrics"
FP32_OPS_PER_S = 157.3e12
# fp32 operations per averaged output / per gradient pixel, counted from csrc/ssim_loss.hip: forward vertical pass 5 moments x 11
# taps x 2 = 110, horizontal 110, S 20, the three maps 30; backward 3 maps x (22 + 22) and 10 for the combination
FWD_OPS, FWD_SAVE_OPS, BWD_OPS = 240, 270, 142


def note(msg):
    print(msg, file=sys.stderr, flush=True)


def window_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def alternate(fns, calls, reps, warmup):
    """fns: {name: fn}; per name the per-call ms of `reps` windows, the windows of the different names interleaved."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(window_ms(fn, calls[k]))
    stat = lambda v: {"median_ms": round(sorted(v)[len(v) // 2], 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    return {k: stat(v) for k, v in times.items()}


def held_bytes(forward):
    """Device bytes alive after `forward()` (its result kept) minus before: what waits for the backward."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = forward()
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - before
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return int(held), int(peak)


def bench_shape(B, C, H, W, convention, reps, warmup, dev):
    import ssim_loss_ref as R
    from freesplat_amd import ssim_loss as S
    g = torch.Generator(device=dev).manual_seed(H + B)
    gt = torch.rand(B, C, H, W, device=dev, generator=g)
    pred = (gt + 0.05 * torch.randn(B, C, H, W, device=dev, generator=g)).clamp(0, 1).requires_grad_(True)
    lam = 0.2

    def fused_fwd():
        with torch.no_grad():
            return S.photometric_loss(pred, gt, lam, convention)

    def eager_fwd():
        with torch.no_grad():
            return R.photometric_loss(pred, gt, lam, convention)

    def fused_train():
        return torch.autograd.grad(S.photometric_loss(pred, gt, lam, convention), pred)

    def eager_train():
        return torch.autograd.grad(R.photometric_loss(pred, gt, lam, convention), pred)

    fns = {"fused_fwd": fused_fwd, "eager_fwd": eager_fwd, "fused_fwd_bwd": fused_train, "eager_fwd_bwd": eager_train}
    calls = {"fused_fwd": 40, "eager_fwd": 6, "fused_fwd_bwd": 40, "eager_fwd_bwd": 4}
    t = alternate(fns, calls, reps, warmup)
    lf, le = float(fused_fwd()), float(eager_fwd())
    gf, ge = fused_train()[0], eager_train()[0]
    held_f, peak_f = held_bytes(lambda: S.photometric_loss(pred, gt, lam, convention))
    held_e, peak_e = held_bytes(lambda: R.photometric_loss(pred, gt, lam, convention))
    px = B * C * H * W
    outs = px if convention == "3dgs" else B * C * (H - 10) * (W - 10)
    b_fwd, b_fwd_save, b_bwd = 8 * px, 8 * px + 12 * outs, 12 * outs + 12 * px
    ops_fwd, ops_train = FWD_OPS * outs, FWD_SAVE_OPS * outs + BWD_OPS * px
    ms_f, ms_t = t["fused_fwd"]["median_ms"], t["fused_fwd_bwd"]["median_ms"]
    row = {
        "views": B, "C": C, "H": H, "W": W, "convention": convention, "lambda_dssim": lam, **{k: v for k, v in t.items()},
        "fwd_speedup": round(t["eager_fwd"]["median_ms"] / ms_f, 2),
        "fwd_bwd_speedup": round(t["eager_fwd_bwd"]["median_ms"] / ms_t, 2),
        "held_for_backward_bytes": {"fused": held_f, "eager": held_e, "fused_saved_bytes_query": S.saved_bytes(B, C, H, W, convention)},
        "peak_bytes_above_inputs_during_forward": {"fused": peak_f, "eager": peak_e},
        "algorithmic": {"fwd_bytes": b_fwd, "fwd_bwd_bytes": b_fwd_save + b_bwd, "fwd_fp32_ops": ops_fwd, "fwd_bwd_fp32_ops": ops_train},
        # whole-call time (two launches plus the [B]-tensor torch glue), not kernel time: a floor on the kernels' share of peak
        "fwd_call_share_of_hbm_peak": round(b_fwd / HBM_BYTES_PER_S / (1e-3 * ms_f), 3),
        "fwd_call_share_of_fp32_peak": round(ops_fwd / FP32_OPS_PER_S / (1e-3 * ms_f), 3),
        "fwd_bwd_call_share_of_hbm_peak": round((b_fwd_save + b_bwd) / HBM_BYTES_PER_S / (1e-3 * ms_t), 3),
        "fwd_bwd_call_share_of_fp32_peak": round(ops_train / FP32_OPS_PER_S / (1e-3 * ms_t), 3),
        "parity": {"loss_abs_diff_vs_eager": abs(lf - le), "grad_rel_diff_vs_eager": float((gf - ge).abs().max() / ge.abs().max())},
    }
    note(json.dumps(row))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ssim_loss_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ssim_loss.py needs a HIP device (no CPU fallback)")
    dev = torch.device("cuda:0")
    out = {"bench": "ssim_loss", "device": torch.cuda.get_device_name(0), "baseline": "eager fp32 torch restatement "
           "(tests/ssim_loss_ref.py: grouped separable conv2d under autograd) on the same device, same session, alternated windows",
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "fp32_ops_per_s": FP32_OPS_PER_S, "reps": args.reps, "warmup": args.warmup, "rows": []}
    for B, C, H, W in SIZES:
        for convention in ("3dgs", "skimage"):
            out["rows"].append(bench_shape(B, C, H, W, convention, args.reps, args.warmup, dev))
    out["fused_never_slower"] = all(r["fwd_speedup"] >= 1.0 and r["fwd_bwd_speedup"] >= 1.0 for r in out["rows"])
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
