#!/usr/bin/env python
"""Normals-loss benchmark (standalone; not the headline metric).  One process, every shape warmed first.

  fused    freesplat_amd.normals_loss.normals_loss (fs_normals_loss_forward / _backward), forward under no_grad and forward +
           backward to depth (and alpha), as ms per call including the Python wrapper
  eager    the same loss as a user writes it today: tests/normals_loss_ref.py in float32 on the same device (clamped gathers for
           the blur and the Sobel taps, cross product, F.normalize, masks by NaN propagation, under autograd) -- a yardstick,
           not code under test
for 4 views x 968 x 1296 and 8 x 384 x 512, with and without alpha, a gt_depth target and precomputed gt_normals, smoothing 2.0
and None, 20 % holes in the target (16 x 16 blocks; the share of pixels that enter the loss is reported).  Fused and eager windows alternate inside one session; the median window and the spread
(min, max) of the per-call times are reported, with the two library calls alone (device events around back-to-back calls on
preallocated buffers), the bytes each form holds between forward and backward (torch.cuda.memory_allocated after the forward
minus before it) and the algorithmic byte floor (every input read once per pass, every gradient written once) as a share of
the measured 6.29 TB/s copy rate.

Prints one JSON object and writes it to --out.    python bench_normals_loss.py [--reps 7 --warmup 3 --out profiles/normals_loss_bench.json]
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


def alternate(fns, calls, reps):
    """fns: {name: fn}; per name the per-call ms of `reps` windows, the windows of the different names interleaved."""
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


def library_calls_us(depth, alpha, intr, gt_depth, gt_normals, sigma, calls=30, reps=5):
    """(forward, backward) microseconds per fs_normals_loss_forward / _backward call on preallocated buffers."""
    from freesplat_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    B, H, W = depth.shape
    dev = depth.device
    scratch = torch.empty(L.fs_normals_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    total, cnt = torch.empty(2, B, dtype=torch.float64, device=dev)
    g_sum = torch.ones(B, device=dev)
    g_depth, g_alpha = torch.empty_like(depth), (None if alpha is None else torch.empty_like(depth))
    st, scalars = _lib.current_stream(), (sigma, 0.0, float("inf"), 1e-3)

    def fwd():
        _lib.check(L.fs_normals_loss_forward(B, H, W, p(depth), p(alpha), p(intr), p(gt_depth), p(gt_normals), *scalars, p(total),
                                             p(cnt), p(scratch), st), "fs_normals_loss_forward")

    def bwd():
        _lib.check(L.fs_normals_loss_backward(B, H, W, p(depth), p(alpha), p(intr), p(gt_depth), p(gt_normals), *scalars, p(g_sum),
                                              p(g_depth), p(g_alpha), st), "fs_normals_loss_backward")

    out = []
    for fn in (fwd, bwd):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        out.append(round(1e3 * sorted(window_ms(fn, calls) for _ in range(reps))[reps // 2], 1))
    return tuple(out)


def make_case(B, H, W, with_alpha, target, smoothing, dev):
    """The closures of one configuration and what the report needs of it."""
    import normals_loss_ref as R
    from freesplat_amd import normals_loss as N
    g = torch.Generator(device=dev).manual_seed(H + B)
    r = lambda: torch.rand(B, H, W, device=dev, generator=g)
    y = torch.arange(H, device=dev).view(1, H, 1) / H
    x = torch.arange(W, device=dev).view(1, 1, W) / W
    gt = 2.25 + 0.4 * torch.sin(7.0 * x + 1.0) + 0.3 * torch.cos(5.0 * y) + 0.005 * torch.randn(B, H, W, device=dev, generator=g)
    E = gt * (1.0 + 0.02 * torch.sin(23.0 * x * y)) + 0.005 * torch.randn(B, H, W, device=dev, generator=g)
    # 20 % holes, in 16 x 16 blocks as a sensor leaves them (single-pixel holes at that rate would leave the 7 x 7 windows of the
    # smoothed form almost nothing to work on)
    coarse = torch.rand(B, -(-H // 16), -(-W // 16), device=dev, generator=g) < 0.2
    hole = coarse.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :H, :W]
    gt = torch.where(hole, torch.full_like(gt, float("nan")), gt)
    intr = torch.tensor([[0.8 * W, 0.8 * W, 0.48 * W, 0.51 * H]], device=dev).expand(B, 4).contiguous()
    alpha = (0.3 + 0.7 * r()).requires_grad_(True) if with_alpha else None
    depth = (E * alpha.detach() if with_alpha else E).requires_grad_(True)
    leaves = [depth, alpha] if with_alpha else [depth]
    if target == "gt_depth":
        tkw = dict(gt_depth=gt)
    else:
        with torch.no_grad():                                                    # the sensor's normals, once per view
            tkw = dict(gt_normals=N.depth_normals(gt, intr, smoothing=smoothing))
    kw = dict(alpha=alpha, smoothing=smoothing, **tkw)

    def fused_fwd():
        with torch.no_grad():
            return N.normals_loss(depth, intr, **kw)

    def eager_fwd():
        with torch.no_grad():
            return R.normals_loss(depth, intr, **kw)

    def fused_train():
        return torch.autograd.grad(N.normals_loss(depth, intr, **kw), leaves)

    def eager_train():
        return torch.autograd.grad(R.normals_loss(depth, intr, **kw), leaves)

    fns = {"fused_fwd": fused_fwd, "eager_fwd": eager_fwd, "fused_fwd_bwd": fused_train, "eager_fwd_bwd": eager_train}
    held = {"fused": lambda: N.normals_loss(depth, intr, **kw), "eager": lambda: R.normals_loss(depth, intr, **kw),
            "cnt": lambda: N.normals_loss_terms(depth.detach(), intr, **dict(kw, alpha=None if alpha is None else alpha.detach()))[1].sum() / (B * H * W)}
    lib = lambda: library_calls_us(depth.detach(), None if alpha is None else alpha.detach(), intr, tkw.get("gt_depth"),
                                   tkw.get("gt_normals"), 0.0 if smoothing is None else float(smoothing))
    return fns, held, lib


def report(B, H, W, with_alpha, target, smoothing, case, reps):
    fns, held, lib = case
    calls = {"fused_fwd": 40, "eager_fwd": 4, "fused_fwd_bwd": 40, "eager_fwd_bwd": 3}
    t = alternate(fns, calls, reps)
    lf, le = float(fns["fused_fwd"]()), float(fns["eager_fwd"]())
    valid = float(held["cnt"]())
    gf, ge = fns["fused_fwd_bwd"](), fns["eager_fwd_bwd"]()
    held_f, peak_f = held_bytes(held["fused"])
    held_e, peak_e = held_bytes(held["eager"])
    lib_fwd, lib_bwd = lib()
    px = B * H * W
    n_in = 1 + (1 if with_alpha else 0) + (1 if target == "gt_depth" else 3)
    n_out = 2 if with_alpha else 1
    b_fwd, b_train = 4 * n_in * px, 4 * (2 * n_in + n_out) * px
    ms_f, ms_t = t["fused_fwd"]["median_ms"], t["fused_fwd_bwd"]["median_ms"]
    row = {
        "views": B, "H": H, "W": W, "alpha": with_alpha, "target": target, "smoothing": smoothing, "pixels_in_the_loss": round(valid, 3),
        **{k: v for k, v in t.items()},
        "fwd_speedup": round(t["eager_fwd"]["median_ms"] / ms_f, 2),
        "fwd_bwd_speedup": round(t["eager_fwd_bwd"]["median_ms"] / ms_t, 2),
        "held_for_backward_bytes": {"fused": held_f, "eager": held_e},
        "peak_bytes_above_inputs_during_forward": {"fused": peak_f, "eager": peak_e},
        "algorithmic_floor_bytes": {"fwd": b_fwd, "fwd_bwd": b_train},
        # the two library calls alone, without the autograd wrapper and the torch glue: events around 30 back-to-back calls
        # (2 launches resp. 1), i.e. the larger of their device time and their enqueue time
        "library_call_us": {"fwd": lib_fwd, "bwd": lib_bwd},
        "library_calls_share_of_hbm_copy_rate": round(b_train / HBM_BYTES_PER_S / (1e-6 * (lib_fwd + lib_bwd)), 3),
        # whole-call time (all launches plus the [B]-tensor torch glue), not kernel time
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_loss_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_normals_loss.py needs a HIP device (no CPU fallback)")
    dev = torch.device("cuda:0")
    out = {"bench": "normals_loss", "device": torch.cuda.get_device_name(0), "baseline": "eager fp32 torch restatement "
           "(tests/normals_loss_ref.py: clamped gathers, cross product and F.normalize under autograd) on the same device, same "
           "session, alternated windows", "hbm_bytes_per_s": HBM_BYTES_PER_S, "reps": args.reps, "warmup": args.warmup, "rows": []}
    configs = [(B, H, W, with_alpha, target, smoothing) for B, H, W in SIZES for with_alpha in (True, False)
               for target in ("gt_depth", "gt_normals") for smoothing in (2.0, None)]
    # every shape and configuration is warmed before the first timed window
    for cfg in configs:
        fns, _, _ = make_case(*cfg, dev)
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        del fns
    torch.cuda.synchronize()
    for cfg in configs:
        case = make_case(*cfg, dev)
        for fn in case[0].values():
            fn()
        torch.cuda.synchronize()
        out["rows"].append(report(*cfg, case, args.reps))
        del case
        torch.cuda.empty_cache()
    out["fused_never_slower"] = all(r["fwd_speedup"] >= 1.0 and r["fwd_bwd_speedup"] >= 1.0 for r in out["rows"])
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
