#!/usr/bin/env python
"""Gaussian Adam benchmark (standalone; not the headline metric): the parameter update of per-scene refinement at 1.0 M
Gaussians, SH degree 3 (M = 16, 59 floats per Gaussian).  One process, everything warmed first.

  fused     freesplat_amd.refine.GaussianAdam.step (fs_gaussian_adam_step): chain rule through exp / sigmoid, Adam over the
            five arrays and the activation of the result in one launch; dense, and sparse with 10 %, 30 % and 100 % of the rows
            visible (rows drawn at random, the hardest pattern for a skip: neighbours in memory rarely share their fate)
  baseline  what a user writes today: log-scales and logits as torch leaves, `exp` / `sigmoid` eagerly on every step, autograd
            through them for the two raw gradients, then torch.optim.Adam over the five tensors -- default (foreach),
            fused=True and capturable=True.  A yardstick, not code under test.
Every form starts from the same gradient buffers (gradients with respect to the activated values, as the rasterizer returns
them).  ms per call INCLUDE the Python wrapper: device events around windows of back-to-back calls, the windows of the
different forms alternated inside one session; the median window and the spread (min, max) are reported, with the algorithmic
bytes of a step and their share of the measured 6.29 TB/s copy rate.

Acceptance: both sides are one pass over the bytes, so the dense fused step must not be slower than the fused=True baseline
(optimizer + activation chain) by more than that baseline's own window spread; the process exits 1 otherwise.

Prints one JSON object and writes it to --out.    python bench_refine.py [--reps 7 --warmup 3 --out profiles/gaussian_adam_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch

N, M = 1_000_000, 16
HBM_BYTES_PER_S = 6.29e12          # measured float4 copy rate (DESIGN.md "Evaluation metrics" uses the same figure)
FLOATS = 3 + 3 + 4 + 1 + 3 * M     # per Gaussian


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


def step_bytes(n, visible_fraction=None):
    """Algorithmic bytes of one step: p, g, m, v read and p, m, v written (28 B per parameter), the activated scales and
    opacities written (4 floats per Gaussian); a sparse step moves that for the visible rows and reads radii for all."""
    dense = 28 * FLOATS * n + 16 * n
    return dense if visible_fraction is None else int(visible_fraction * dense) + 4 * n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gaussians", type=int, default=N)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussian_adam_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_refine.py needs a HIP device (no CPU fallback)")
    from freesplat_amd.refine import GaussianAdam
    dev = torch.device("cuda:0")
    n = args.gaussians
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)
    shapes = [(n, 3), (n, 3), (n, 4), (n, 1), (n, M, 3)]
    raw = [rnd(n, 3), rnd(n, 3) - 4.0, rnd(n, 4), rnd(n, 1).clamp(-6, 6), 0.3 * rnd(n, M, 3)]
    grads = [1e-3 * rnd(*s) for s in shapes]              # gradients with respect to the activated values, reused by every form
    fns, calls = {}, {}

    # ---- fused: one optimizer per variant, so that every form owns its state
    def fused(sparse, fraction):
        opt = GaussianAdam(raw[0], torch.exp(raw[1]), raw[2], torch.sigmoid(raw[3]), raw[4], sparse=sparse)
        radii = None
        if sparse:
            radii = (torch.rand(n, device=dev, generator=gen) < fraction).to(torch.int32) * 5
        leaves = opt.leaves()

        def step():
            for leaf, g in zip(leaves, grads):
                leaf.grad = g
            opt.step(radii)
        return step

    fns["fused_dense"], calls["fused_dense"] = fused(False, None), 400
    for pct in (10, 30, 100):
        fns[f"fused_sparse_{pct}"], calls[f"fused_sparse_{pct}"] = fused(True, pct / 100.0), 400

    # ---- baselines: torch.optim.Adam over five tensors with the eager activation chain
    def baseline(**kw):
        leaves = [t.clone().requires_grad_(True) for t in raw]
        lrs = (1.6e-4, 5e-3, 1e-3, 5e-2, 2.5e-3)
        opt = torch.optim.Adam([dict(params=[p], lr=lr) for p, lr in zip(leaves, lrs)], betas=(0.9, 0.999), eps=1e-15, **kw)
        keep = {}

        def step():
            scales, opac = torch.exp(leaves[1]), torch.sigmoid(leaves[3])          # what the next forward consumes
            torch.autograd.backward([scales, opac], [grads[1], grads[3]])
            leaves[0].grad, leaves[2].grad, leaves[4].grad = grads[0], grads[2], grads[4]
            opt.step()
            opt.zero_grad(set_to_none=True)
            keep["acts"] = (scales, opac)
        return step

    errors = {}
    for name, kw in (("adam_default", {}), ("adam_fused", dict(fused=True)), ("adam_capturable", dict(capturable=True))):
        try:
            fn = baseline(**kw)
            fn()
            torch.cuda.synchronize()
            fns["baseline_" + name], calls["baseline_" + name] = fn, 100
        except Exception as e:  # a baseline this torch build cannot run is reported, not hidden
            errors["baseline_" + name] = f"{type(e).__name__}: {e}"
            note(f"baseline {name} unavailable: {errors['baseline_' + name]}")

    t = alternate(fns, calls, args.reps, args.warmup)
    rows = {}
    for k, v in t.items():
        frac = None if not k.startswith("fused_sparse_") else int(k.rsplit("_", 1)[1]) / 100.0
        b = step_bytes(n, frac)
        rows[k] = dict(v, calls_per_window=calls[k], algorithmic_bytes=b,
                       share_of_measured_copy_rate=round(b / HBM_BYTES_PER_S / (1e-3 * v["median_ms"]), 3))
        note(f"{k}: {json.dumps(rows[k])}")
    out = {"bench": "gaussian_adam", "device": torch.cuda.get_device_name(0), "gaussians": n, "sh_coefficients": M,
           "floats_per_gaussian": FLOATS, "hbm_bytes_per_s": HBM_BYTES_PER_S, "reps": args.reps, "warmup": args.warmup,
           "timing": "ms per call including the Python wrapper; device events around windows of back-to-back calls, windows of "
                     "the forms alternated; median (min, max) over the windows",
           "floor_ms_dense": round(1e3 * step_bytes(n) / HBM_BYTES_PER_S, 4), "rows": rows, "baseline_errors": errors}
    ok = None
    if "baseline_adam_fused" in rows:
        base = rows["baseline_adam_fused"]
        spread = base["max_ms"] - base["min_ms"]
        ok = rows["fused_dense"]["median_ms"] <= base["median_ms"] + spread
        out["acceptance"] = {"fused_dense_median_ms": rows["fused_dense"]["median_ms"], "baseline_adam_fused_median_ms": base["median_ms"],
                            "baseline_window_spread_ms": round(spread, 4), "dense_not_slower_than_fused_baseline": bool(ok)}
        for k in rows:
            if k.startswith("baseline_"):
                out.setdefault("speedup_of_fused_dense_over", {})[k] = round(rows[k]["median_ms"] / rows["fused_dense"]["median_ms"], 2)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    if not ok:
        raise SystemExit("bench_refine.py: the dense fused step is slower than the fused=True baseline beyond its window spread "
                         "(or that baseline could not run)")


if __name__ == "__main__":
    main()
