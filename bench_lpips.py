#!/usr/bin/env python
"""LPIPS benchmark (standalone; not the headline metric).  Random weights, one process, every shape warmed first.

  head alone   the fused distance head (fs_lpips_layer_forward / _backward) against the eager fp32 torch head on the same
               tensors (tests/lpips_ref.py in float32: what a user has today, not code under test), forward and
               forward + backward to the prediction's map, on the five VGG-16 tap shapes of 4 pairs at 968x1296 and of
               8 pairs at 384x512; bytes moved and the share of the one-read floor (bytes / 6.0 TB/s)
  whole term   prepare -> VGG-16 -> head -> backward to the prediction (freesplat_amd.lpips.LPIPS), the same with the eager
               head, and the VGG-16 stack alone (forward of both halves, backward of the prediction's), so that the
               head's share of the term can be read off; torch.cuda.max_memory_allocated of the term

Prints one JSON object.    python bench_lpips.py [--reps 20 --warmup 3 --term-reps 5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch

SIZES = [(4, 968, 1296), (8, 384, 512)]          # (pairs, H, W): config 3's four targets; the native context size
TAPS = [(64, 1), (128, 2), (256, 4), (512, 8), (512, 16)]
STREAM_BYTES_PER_S = 6.0e12                       # measured streaming rate of the part (MI355X guide)


def note(msg):
    print(msg, file=sys.stderr, flush=True)


def gpu_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(3):                            # three windows of `reps` calls; the median window is reported
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / reps)
    return sorted(times)[1]


def head_bytes(B, C, h, w):
    maps, saved = 2 * B * C * h * w * 4, 16 * B * h * w
    fwd = maps + saved                            # one read of both maps, four floats per pixel written
    return fwd, fwd + maps + saved + maps // 2    # + one more read of both, the saved floats, one gradient written


def bench_head(B, H, W, reps, warmup, dev):
    import lpips_ref as R
    from freesplat_amd.lpips import lpips_head
    rows = []
    for C, s in TAPS:
        h, w = H // s, W // s
        g = torch.Generator(device=dev).manual_seed(C + h)
        f0 = torch.relu(torch.randn(B, C, h, w, device=dev, generator=g)).requires_grad_(True)
        f1 = torch.relu(torch.randn(B, C, h, w, device=dev, generator=g))
        lw = torch.rand(C, device=dev, generator=g)

        def fused_fwd():
            with torch.no_grad():
                return lpips_head([f0], [f1], [lw])

        def fused_train():
            return torch.autograd.grad(lpips_head([f0], [f1], [lw]).sum(), f0)

        def eager_fwd():
            with torch.no_grad():
                return R.layer(f0, f1, lw, torch.float32)

        def eager_train():
            return torch.autograd.grad(R.layer(f0, f1, lw, torch.float32).sum(), f0)

        t = {k: gpu_ms(fn, reps, warmup) for k, fn in (("fused_fwd", fused_fwd), ("eager_fwd", eager_fwd),
                                                      ("fused_fwd_bwd", fused_train), ("eager_fwd_bwd", eager_train))}
        d_f, d_e = fused_fwd(), eager_fwd()
        b_fwd, b_train = head_bytes(B, C, h, w)
        rows.append({
            "C": C, "h": h, "w": w,
            "fused_fwd_ms": round(t["fused_fwd"], 4), "eager_fwd_ms": round(t["eager_fwd"], 4),
            "fwd_speedup": round(t["eager_fwd"] / t["fused_fwd"], 2),
            "fused_fwd_bwd_ms": round(t["fused_fwd_bwd"], 4), "eager_fwd_bwd_ms": round(t["eager_fwd_bwd"], 4),
            "fwd_bwd_speedup": round(t["eager_fwd_bwd"] / t["fused_fwd_bwd"], 2),
            "fwd_bytes": b_fwd, "fwd_bwd_bytes": b_train,
            "fwd_share_of_one_read_floor": round(b_fwd / STREAM_BYTES_PER_S / (1e-3 * t["fused_fwd"]), 3),
            "fwd_bwd_share_of_one_read_floor": round(b_train / STREAM_BYTES_PER_S / (1e-3 * t["fused_fwd_bwd"]), 3),
            "parity_rel": float(((d_f - d_e).abs() / d_e.abs()).max()),
        })
        note(f"head {B}x{C}x{h}x{w}: {rows[-1]}")
        del f0, f1
        torch.cuda.empty_cache()
    tot = lambda k: round(sum(r[k] for r in rows), 4)
    return {"pairs": B, "H": H, "W": W, "taps": rows,
            "sum_fused_fwd_ms": tot("fused_fwd_ms"), "sum_eager_fwd_ms": tot("eager_fwd_ms"),
            "sum_fused_fwd_bwd_ms": tot("fused_fwd_bwd_ms"), "sum_eager_fwd_bwd_ms": tot("eager_fwd_bwd_ms")}


def bench_term(B, H, W, reps, warmup, dev):
    import lpips_ref as R
    from freesplat_amd.lpips import LPIPS, _Prepare
    m = LPIPS(net="vgg", weights="random", seed=0).to(dev)
    g = torch.Generator(device=dev).manual_seed(H)
    target = torch.rand(B, 3, H, W, device=dev, generator=g)
    pred = (target + 0.05 * torch.randn(B, 3, H, W, device=dev, generator=g)).clamp(0, 1).requires_grad_(True)
    ws = m.lin_weights()
    shift, scale = m.scaling_layer.shift.reshape(-1), m.scaling_layer.scale.reshape(-1)

    def term():
        return torch.autograd.grad(m(pred, target).mean(), pred)

    def taps_of(x):
        with torch.no_grad():
            t1 = m.net(x[B:])
        return m.net(x[:B]), t1

    def term_eager_head():
        t0, t1 = taps_of(_Prepare.apply(pred, target, shift, scale, False))
        return torch.autograd.grad(R.head(t0, t1, ws, torch.float32).mean(), pred)

    t0, _ = taps_of(_Prepare.apply(pred, target, shift, scale, False))
    g_taps = [torch.randn_like(t) for t in t0]
    del t0

    def vgg_only():
        t0, _ = taps_of(_Prepare.apply(pred, target, shift, scale, False))
        return torch.autograd.grad(t0, pred, g_taps)

    def vgg_forward():
        with torch.no_grad():
            return m.net(_Prepare.apply(pred, target, shift, scale, False))

    torch.cuda.reset_peak_memory_stats()
    out = {"pairs": B, "H": H, "W": W}
    out["term_ms"] = round(gpu_ms(term, reps, warmup), 3)
    out["term_max_memory_allocated_GB"] = round(torch.cuda.max_memory_allocated() / 1e9, 3)
    note(f"term {B}x{H}x{W}: {out}")
    out["term_eager_head_ms"] = round(gpu_ms(term_eager_head, reps, warmup), 3)
    out["vgg_fwd_bwd_ms"] = round(gpu_ms(vgg_only, reps, warmup), 3)
    out["vgg_fwd_only_2B_images_ms"] = round(gpu_ms(vgg_forward, reps, warmup), 3)
    out["head_and_prepare_ms"] = round(out["term_ms"] - out["vgg_fwd_bwd_ms"], 3)
    out["head_share_of_term"] = round(out["head_and_prepare_ms"] / out["term_ms"], 4)
    out["eager_head_share_of_its_term"] = round((out["term_eager_head_ms"] - out["vgg_fwd_bwd_ms"]) / out["term_eager_head_ms"], 4)
    note(f"term {B}x{H}x{W}: {out}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--term-reps", type=int, default=5)
    ap.add_argument("--skip-term", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips.py needs a HIP device (no CPU fallback)")
    dev = torch.device("cuda:0")
    out = {"bench": "lpips", "weights": "random", "stream_bytes_per_s": STREAM_BYTES_PER_S,
           "device": torch.cuda.get_device_name(0), "head": [], "term": []}
    for B, H, W in SIZES:
        out["head"].append(bench_head(B, H, W, args.reps, args.warmup, dev))
    if not args.skip_term:
        for B, H, W in SIZES:
            out["term"].append(bench_term(B, H, W, args.term_reps, 2, dev))
    out["fused_head_never_slower"] = all(r["fwd_speedup"] >= 1.0 and r["fwd_bwd_speedup"] >= 1.0
                                         for s in out["head"] for r in s["taps"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
