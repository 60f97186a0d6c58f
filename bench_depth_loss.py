#!/usr/bin/env python
"""Depth-loss benchmark (standalone; not the headline metric).  One process, every shape warmed first.

  fused    freesplat_amd.depth_loss.depth_loss (fs_depth_loss_forward / _backward), forward under no_grad and forward +
           backward to depth (and alpha), as ms per call including the Python wrapper
  eager    the same loss as a user writes it today: tests/depth_loss_ref.py in float32 on the same device (stride-2 and
           replicate-padded conv2d, masks by NaN propagation, under autograd) -- a yardstick, not code under test
for 4 views x 968 x 1296 and 8 x 384 x 512, log-L1 point term, 4 scales, with and without alpha, 20 % holes in the ground
truth.  Fused and eager windows alternate inside one session; the median window and the spread (min, max) of the per-call
times are reported, with the bytes each form holds between forward and backward (torch.cuda.memory_allocated after the
forward minus before it) and the algorithmic byte floor (every input read once per pass, every gradient written once) as a
share of the measured 6.29 TB/s copy rate.

Prints one JSON object and writes it to --out.    python bench_depth_loss.py [--reps 7 --warmup 3 --out profiles/depth_loss_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch

SIZES = [(4, 968, 1296), (8, 384, 512)]
HBM_BYTES_PER_S = 6.29e12          # measured float4 copy rate (DESIGN.md "Evaluation metrics")
SCALES = 4


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


def library_calls_us(depth, gt, alpha, calls=30, reps=5):
    """(forward, backward) microseconds per fs_depth_loss_forward / _backward call on preallocated buffers."""
    from freesplat_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    B, H, W = depth.shape
    dev = depth.device
    scratch = torch.empty(L.fs_depth_loss_scratch_bytes(B, H, W, SCALES), dtype=torch.uint8, device=dev)
    saved = torch.empty(L.fs_depth_loss_saved_bytes(B, H, W, SCALES), dtype=torch.uint8, device=dev)
    ps, pc = torch.empty(2, B, dtype=torch.float64, device=dev)
    gs, gc = torch.empty(2, B, SCALES, dtype=torch.float64, device=dev)
    g_point, g_grad = torch.ones(B, device=dev), torch.ones(B, SCALES, device=dev)
    g_depth, g_alpha = torch.empty_like(depth), (None if alpha is None else torch.empty_like(depth))
    st, scalars = _lib.current_stream(), (0.0, float("inf"), 1e-3)
    mode = _lib.DEPTH_LOSS_LOG_L1

    def fwd():
        _lib.check(L.fs_depth_loss_forward(B, H, W, SCALES, mode, p(depth), p(gt), p(alpha), *scalars, p(ps), p(pc), p(gs), p(gc),
                                           p(saved), p(scratch), st), "fs_depth_loss_forward")

    def bwd():
        _lib.check(L.fs_depth_loss_backward(B, H, W, SCALES, mode, p(depth), p(gt), p(alpha), *scalars, p(g_point), p(g_grad),
                                            p(saved), p(g_depth), p(g_alpha), p(scratch), st), "fs_depth_loss_backward")

    out = []
    for fn in (fwd, bwd):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        out.append(round(1e3 * sorted(window_ms(fn, calls) for _ in range(reps))[reps // 2], 1))
    return tuple(out)


def bench_shape(B, H, W, with_alpha, reps, warmup, dev):
    import depth_loss_ref as R
    from freesplat_amd import depth_loss as D
    g = torch.Generator(device=dev).manual_seed(H + B)
    r = lambda: torch.rand(B, H, W, device=dev, generator=g)
    gt = 0.5 + 4.0 * r()
    E = gt * torch.exp(0.1 * torch.randn(B, H, W, device=dev, generator=g))
    gt = torch.where(r() < 0.2, torch.full_like(gt, float("nan")), gt)
    alpha = (0.3 + 0.7 * r()).requires_grad_(True) if with_alpha else None
    depth = (E * alpha.detach() if with_alpha else E).requires_grad_(True)
    leaves = [depth, alpha] if with_alpha else [depth]
    kw = dict(mode="log_l1", num_scales=SCALES)

    def fused_fwd():
        with torch.no_grad():
            return D.depth_loss(depth, gt, alpha, **kw)

    def eager_fwd():
        with torch.no_grad():
            return R.depth_loss(depth, gt, alpha, **kw)

    def fused_train():
        return torch.autograd.grad(D.depth_loss(depth, gt, alpha, **kw), leaves)

    def eager_train():
        return torch.autograd.grad(R.depth_loss(depth, gt, alpha, **kw), leaves)

    fns = {"fused_fwd": fused_fwd, "eager_fwd": eager_fwd, "fused_fwd_bwd": fused_train, "eager_fwd_bwd": eager_train}
    calls = {"fused_fwd": 40, "eager_fwd": 6, "fused_fwd_bwd": 40, "eager_fwd_bwd": 4}
    t = alternate(fns, calls, reps, warmup)
    lf, le = float(fused_fwd()), float(eager_fwd())
    gf, ge = fused_train(), eager_train()
    held_f, peak_f = held_bytes(lambda: D.depth_loss(depth, gt, alpha, **kw))
    held_e, peak_e = held_bytes(lambda: R.depth_loss(depth, gt, alpha, **kw))
    lib_fwd, lib_bwd = library_calls_us(depth.detach(), gt, None if alpha is None else alpha.detach())
    px = B * H * W
    n_in, n_out = (3, 2) if with_alpha else (2, 1)
    b_fwd, b_train = 4 * n_in * px, 4 * (2 * n_in + n_out) * px
    ms_f, ms_t = t["fused_fwd"]["median_ms"], t["fused_fwd_bwd"]["median_ms"]
    row = {
        "views": B, "H": H, "W": W, "alpha": with_alpha, "mode": "log_l1", "num_scales": SCALES, **{k: v for k, v in t.items()},
        "fwd_speedup": round(t["eager_fwd"]["median_ms"] / ms_f, 2),
        "fwd_bwd_speedup": round(t["eager_fwd_bwd"]["median_ms"] / ms_t, 2),
        "held_for_backward_bytes": {"fused": held_f, "eager": held_e, "fused_saved_bytes_query": D.saved_bytes(B, H, W, SCALES)},
        "peak_bytes_above_inputs_during_forward": {"fused": peak_f, "eager": peak_e},
        "algorithmic_floor_bytes": {"fwd": b_fwd, "fwd_bwd": b_train},
        # the two library calls alone, without the autograd wrapper and the torch glue: events around 30 back-to-back calls
        # (S + 1 resp. S launches each), i.e. the larger of their device time and their enqueue time
        "library_call_us": {"fwd": lib_fwd, "bwd": lib_bwd},
        "library_calls_share_of_hbm_copy_rate": round(b_train / HBM_BYTES_PER_S / (1e-6 * (lib_fwd + lib_bwd)), 3),
        # whole-call time (all launches plus the [B] / [B, S]-tensor torch glue), not kernel time
        "fwd_call_share_of_hbm_copy_rate": round(b_fwd / HBM_BYTES_PER_S / (1e-3 * ms_f), 3),
        "fwd_bwd_call_share_of_hbm_copy_rate": round(b_train / HBM_BYTES_PER_S / (1e-3 * ms_t), 3),
        "parity": {"loss_abs_diff_vs_eager": abs(lf - le),
                   "grad_rel_diff_vs_eager": max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(gf, ge))},
    }
    note(json.dumps(row))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_loss_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth_loss.py needs a HIP device (no CPU fallback)")
    dev = torch.device("cuda:0")
    out = {"bench": "depth_loss", "device": torch.cuda.get_device_name(0), "baseline": "eager fp32 torch restatement "
           "(tests/depth_loss_ref.py: conv2d pyramid and Sobel pass under autograd) on the same device, same session, alternated windows",
           "hbm_bytes_per_s": HBM_BYTES_PER_S, "reps": args.reps, "warmup": args.warmup, "rows": []}
    for B, H, W in SIZES:
        for with_alpha in (True, False):
            out["rows"].append(bench_shape(B, H, W, with_alpha, args.reps, args.warmup, dev))
    out["fused_never_slower"] = all(r["fwd_speedup"] >= 1.0 and r["fwd_bwd_speedup"] >= 1.0 for r in out["rows"])
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
