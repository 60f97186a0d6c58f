#!/usr/bin/env python
"""Exposure-compensation benchmark (standalone; not the headline metric).  One process, every shape warmed first.

  fused    freesplat_amd.exposure: apply_exposure under no_grad, apply_exposure + backward (both gradients, and the parameters'
           alone), fit_exposure with a mask -- ms per call including the Python wrapper
  eager    what a user writes today, in fp32 torch on the same device (tests/exposure_ref.py eager_apply / eager_fit): einsum +
           broadcast add under autograd for the apply, masked fp64 normal equations + torch.linalg.solve for the fit -- a
           yardstick, not code under test
for 4 views x 3 x 968 x 1296 and 8 x 3 x 384 x 512, one view per entry.  Fused and eager windows alternate inside one session; the
median window and the spread (min, max) of the per-call times are reported, with each library call alone (device events around
back-to-back calls on preallocated buffers), the bytes each form holds between forward and backward (torch.cuda.memory_allocated
after the forward minus before it) and each library call's algorithmic byte floor over its time as a share of the copy rate
measured in the same session (a 1 GiB float4 copy, read + written bytes; the copy of one image-sized array is reported too: at
these sizes a call's whole footprint fits the chip's last-level cache).

Prints one JSON object and writes it to --out.    python bench_exposure.py [--reps 7 --warmup 3 --out profiles/exposure_bench.json]
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
    """Device bytes alive after `forward()` (its result kept) minus before, minus the result itself: what waits for the
    backward beyond the inputs and the output; and the peak during the forward, the result included."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = forward()
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - before - out.numel() * out.element_size()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return {"held": int(held), "forward_peak": int(peak)}


def copy_rate(nbytes, reps=7, calls=10):
    """Read + written bytes per second of a device-to-device copy of `nbytes`."""
    src = torch.empty(nbytes // 16, 4, device="cuda").normal_()
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    torch.cuda.synchronize()
    ms = sorted(window_ms(lambda: dst.copy_(src), calls) for _ in range(reps))[reps // 2]
    return 2.0 * src.numel() * 4 / (1e-3 * ms)


def library_calls_us(image, params, g_out, target, mask, calls=30, reps=7):
    """Microseconds per library call on preallocated buffers: forward, backward (both gradients / the image's / the parameters'),
    fit with and without the mask."""
    from freesplat_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    B, _, H, W = image.shape
    V, dev = params.shape[0], image.device
    out, g_image, g_params = torch.empty_like(image), torch.empty_like(image), torch.empty_like(params)
    fitted, count, solved = torch.empty_like(params), torch.empty(V, dtype=torch.int64, device=dev), torch.empty(V, dtype=torch.uint8, device=dev)
    scratch = torch.empty(L.fs_exposure_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    st = _lib.current_stream()
    bwd = lambda gi, gp: lambda: _lib.check(L.fs_exposure_apply_backward(B, V, H, W, p(image), p(params), None, p(g_out), p(gi), p(gp),
                                                                         p(scratch), st), "fs_exposure_apply_backward")
    fit = lambda m: lambda: _lib.check(L.fs_exposure_fit(B, V, H, W, p(image), p(target), p(m), None, 1e-6, p(fitted), p(count), p(solved),
                                                         p(scratch), st), "fs_exposure_fit")
    fns = {"fwd": lambda: _lib.check(L.fs_exposure_apply_forward(B, V, H, W, p(image), p(params), None, p(out), st),
                                     "fs_exposure_apply_forward"),
           "bwd_both": bwd(g_image, g_params), "bwd_image": bwd(g_image, None), "bwd_params": bwd(None, g_params),
           "fit_mask": fit(mask), "fit": fit(None)}
    res = {}
    for k, fn in fns.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        res[k] = round(1e3 * sorted(window_ms(fn, calls) for _ in range(reps))[reps // 2], 1)
    return res


def make_case(B, H, W, dev):
    import exposure_ref as R
    from freesplat_amd import exposure as E
    g = torch.Generator(device=dev).manual_seed(H + B)
    image = torch.rand(B, 3, H, W, device=dev, generator=g)
    params = (R.identity(B, torch.float32).to(dev) + 0.1 * torch.randn(B, 3, 4, device=dev, generator=g)).contiguous()
    target = (R.eager_apply(image, params) + 0.02 * torch.randn(B, 3, H, W, device=dev, generator=g)).contiguous()
    coarse = torch.rand(B, -(-H // 16), -(-W // 16), device=dev, generator=g) < 0.3          # 30 % out, in 16 x 16 blocks
    mask = ~coarse.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :H, :W].contiguous()
    x, q = image.clone().requires_grad_(True), params.clone().requires_grad_(True)

    def nograd(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run

    fns = {
        "fused_fwd": nograd(lambda: E.apply_exposure(image, params)),
        "eager_fwd": nograd(lambda: R.eager_apply(image, params)),
        "fused_fwd_bwd": lambda: torch.autograd.grad(E.apply_exposure(x, q).square().sum(), [x, q]),
        "eager_fwd_bwd": lambda: torch.autograd.grad(R.eager_apply(x, q).square().sum(), [x, q]),
        "fused_fwd_bwd_params": lambda: torch.autograd.grad(E.apply_exposure(image, q).square().sum(), [q]),
        "eager_fwd_bwd_params": lambda: torch.autograd.grad(R.eager_apply(image, q).square().sum(), [q]),
        "fused_fit": lambda: E.fit_exposure(image, target, mask),
        "eager_fit": lambda: R.eager_fit(image, target, mask),
    }
    held = {"fused": lambda: E.apply_exposure(x, q), "eager": lambda: R.eager_apply(x, q),
            "fused_params": lambda: E.apply_exposure(image, q), "eager_params": lambda: R.eager_apply(image, q)}
    lib = lambda: library_calls_us(image, params, torch.randn_like(image), target, mask.view(torch.uint8))
    return fns, held, lib


def report(B, H, W, case, reps, rate):
    fns, held, lib = case
    calls = {k: (20 if k.startswith("fused") else 5) for k in fns}
    t = alternate(fns, calls, reps)
    # parity of what is timed
    of, oe = fns["fused_fwd"](), fns["eager_fwd"]()
    gf, ge = fns["fused_fwd_bwd"](), fns["eager_fwd_bwd"]()
    pf, pe = fns["fused_fit"]()[0], fns["eager_fit"]()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    lib_us = lib()
    px = B * H * W
    floors = {"fwd": 2 * 12 * px, "bwd_both": 3 * 12 * px, "bwd_image": 2 * 12 * px, "bwd_params": 2 * 12 * px,
              "fit_mask": 2 * 12 * px + px, "fit": 2 * 12 * px}
    speed = lambda name: round(t["eager_" + name]["median_ms"] / t["fused_" + name]["median_ms"], 2)
    row = {
        "views": B, "H": H, "W": W, **t,
        "fwd_speedup": speed("fwd"), "fwd_bwd_speedup": speed("fwd_bwd"), "fwd_bwd_params_speedup": speed("fwd_bwd_params"),
        "fit_speedup": speed("fit"),
        "bytes_beyond_inputs_and_output_held_for_backward_and_forward_peak": {k: held_bytes(v) for k, v in held.items()},
        "algorithmic_floor_bytes": floors,
        # each library call alone, without the autograd wrapper and the torch glue: events around 30 back-to-back calls, i.e. the
        # larger of device time and enqueue time
        "library_call_us": lib_us,
        "library_call_share_of_copy_rate": {k: round(floors[k] / rate / (1e-6 * lib_us[k]), 3) for k in floors},
        "copy_rate_of_one_image_array_bytes_per_s": round(copy_rate(12 * px)),
        "parity": {"out_rel_diff_vs_eager": rel(of, oe), "grad_rel_diff_vs_eager": max(rel(a, b) for a, b in zip(gf, ge)),
                   "fit_rel_diff_vs_eager": rel(pf, pe)},
    }
    note(json.dumps(row))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exposure_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_exposure.py needs a HIP device (no CPU fallback)")
    dev = torch.device("cuda:0")
    rate = copy_rate(1 << 30)
    out = {"bench": "exposure", "device": torch.cuda.get_device_name(0), "baseline": "eager fp32 torch (tests/exposure_ref.py eager_apply: "
           "einsum + broadcast add under autograd; eager_fit: masked fp64 normal equations + torch.linalg.solve) on the same device, "
           "same session, alternated windows", "copy_rate_bytes_per_s": round(rate), "reps": args.reps, "warmup": args.warmup, "rows": []}
    note(f"copy rate {rate / 1e12:.2f} TB/s")
    for cfg in SIZES:                                  # every shape is warmed before the first timed window
        fns, _, _ = make_case(*cfg, dev)
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        del fns
    torch.cuda.synchronize()
    for cfg in SIZES:
        case = make_case(*cfg, dev)
        for fn in case[0].values():
            fn()
        torch.cuda.synchronize()
        out["rows"].append(report(*cfg, case, args.reps, rate))
        del case
        torch.cuda.empty_cache()
    out["fused_never_slower"] = all(r[k] >= 1.0 for r in out["rows"] for k in ("fwd_speedup", "fwd_bwd_speedup", "fwd_bwd_params_speedup",
                                                                                "fit_speedup"))
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
