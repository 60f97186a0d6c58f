#!/usr/bin/env python
"""Skip-branch benchmark (standalone; not the headline metric): the encoder's full-resolution layer Conv2d(3, 64, 7, 1, 3) +
ReLU and the latent pack that consumes it, in one process, at 3 x 968x1296 (BASELINE config 3) and 10 x 384x512.

  chain   what ran before the fused op: torch conv2d (MIOpen) + out-of-place ReLU + gaussian_adapter.latents_pack
  fused   gaussian_adapter.skip_latents (csrc/skip_conv.hip): the same outputs with no [V, 64, H, W] map

forward (no_grad) and forward + backward (gradients of head, weight and bias), device-event timing: every shape warmed, then
`--rounds` windows of `--reps` calls per variant, the two variants alternating window by window; the median window, the
fastest and the slowest are reported, and a variant counts as faster only when its slowest window beats the other's fastest.
Held bytes: what the autograd graph alone keeps between forward and backward (released when the graph goes while the outputs
stay).  Roofline fractions of the fused op: FLOP / 157 TF (the fp32 matrix rate) and algorithmic bytes / 8 TB/s over the time.

Prints one JSON object and writes it to --out.    python bench_skip.py [--reps 200 --rounds 5 --warmup 3 --out profiles/skip_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch

SIZES = [(3, 968, 1296), (10, 384, 512)]
PEAK_FLOPS = 157.3e12
PEAK_BYTES_PER_S = 8.0e12


def note(msg):
    print(msg, file=sys.stderr, flush=True)


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def alternate(fns, reps, rounds, warmup):
    """{name: sorted list of per-call ms, one per window}; the variants take turns window by window."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(window_ms(fn, reps))
    return {k: sorted(v) for k, v in out.items()}


def stats(ms):
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def held_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    lat, dens = fn()
    torch.cuda.synchronize()
    with_graph = torch.cuda.memory_allocated()
    keep = (lat.detach(), dens.detach())
    del lat, dens
    torch.cuda.synchronize()
    held = with_graph - torch.cuda.memory_allocated()
    del keep
    return held


def counts(V, H, W):
    P = V * H * W
    flop = 2 * P * 64 * 147
    fwd = 4 * P * (65 + 3 + 64 + 1)                          # head and image in, latents and densities out
    bwd = 4 * P * (64 + 1 + 65 + 3) + 8 * P                  # g_lat and g_dens in, g_head out, image and the ReLU bits in
    return flop, fwd, fwd + 8 * P + bwd                      # (training forward also writes the bits)


def bench_size(V, H, W, reps, rounds, warmup, dev):
    from freesplat_amd.gaussian_adapter import latents_pack, skip_latents
    g = torch.Generator(device=dev).manual_seed(H)
    torch.manual_seed(H)
    conv = torch.nn.Conv2d(3, 64, 7, 1, 3).to(dev)
    weight, bias = conv.weight, conv.bias
    head = torch.randn(V, 65, H, W, device=dev, generator=g).requires_grad_(True)
    img = torch.rand(V, 3, H, W, device=dev, generator=g)
    g_lat = torch.randn(V, H * W, 64, device=dev, generator=g)
    g_dens = torch.randn(V, H * W, device=dev, generator=g)
    leaves = [head, weight, bias]

    def chain():
        return latents_pack(head, torch.relu(torch.nn.functional.conv2d(img, weight, bias, padding=3)))

    def fused():
        return skip_latents(head, img, weight, bias)

    def fwd(f):
        def run():
            with torch.no_grad():
                return f()
        return run

    def train(f):
        def run():
            lat, dens = f()
            return torch.autograd.grad([lat, dens], leaves, [g_lat, g_dens])
        return run

    t_fwd = alternate({"chain": fwd(chain), "fused": fwd(fused)}, reps, rounds, warmup)
    t_train = alternate({"chain": train(chain), "fused": train(fused)}, reps, rounds, warmup)
    with torch.no_grad():
        parity = float((chain()[0] - fused()[0]).abs().max())
    flop, b_fwd, b_train = counts(V, H, W)
    row = {"V": V, "H": H, "W": W, "flop_per_pass": flop, "fwd_algorithm_bytes": b_fwd, "fwd_bwd_algorithm_bytes": b_train,
           "fwd": {k: stats(v) for k, v in t_fwd.items()}, "fwd_bwd": {k: stats(v) for k, v in t_train.items()},
           "held_bytes": {"chain": held_bytes(chain), "fused": held_bytes(fused), "one_skip_map": V * 64 * H * W * 4},
           "max_abs_difference_of_latents": parity}
    for key, t, passes, nbytes in (("fwd", t_fwd, 1, b_fwd), ("fwd_bwd", t_train, 2, b_train)):
        med = 1e-3 * t["fused"][len(t["fused"]) // 2]
        row[key]["speedup_median"] = round(t["chain"][len(t["chain"]) // 2] / t["fused"][len(t["fused"]) // 2], 3)
        row[key]["fused_faster_beyond_spread"] = t["fused"][-1] < t["chain"][0]
        row[key]["fused_share_of_matrix_floor"] = round(passes * flop / PEAK_FLOPS / med, 3)
        row[key]["fused_share_of_traffic_floor"] = round(nbytes / PEAK_BYTES_PER_S / med, 3)
    note(f"{V}x{H}x{W}: {row}")
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skip_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_skip.py needs a HIP device (no CPU fallback)")
    dev = torch.device("cuda:0")
    out = {"bench": "skip_latents", "device": torch.cuda.get_device_name(0), "peak_flops": PEAK_FLOPS,
           "peak_bytes_per_s": PEAK_BYTES_PER_S, "reps_per_window": args.reps, "windows": args.rounds, "sizes": []}
    for V, H, W in SIZES:
        out["sizes"].append(bench_size(V, H, W, args.reps, args.rounds, args.warmup, dev))
        torch.cuda.empty_cache()
    full = out["sizes"][0]
    out["fused_faster_at_full_size"] = full["fwd"]["fused_faster_beyond_spread"] and full["fwd_bwd"]["fused_faster_beyond_spread"]
    text = json.dumps(out, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
