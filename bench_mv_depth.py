#!/usr/bin/env python
"""Multi-view / scale-invariant depth loss benchmark (standalone; not the headline metric).  One process, every shape warmed
first.

  fused    freesplat_amd.mv_depth_loss.mv_depth_loss and scale_invariant_loss (fs_mv_depth_* / fs_si_depth_*), with alpha,
           forward under no_grad and forward + backward to depth and alpha, as ms per call including the Python wrapper
  eager    the same losses as a user writes them today: tests/mv_depth_ref.py in float32 on the same device (per source a
           projection chain over [B, 3, H, W], a gather, the masks and a masked sum, under autograd) -- a yardstick, not code
           under test
for   a   4 views x 968 x 1296, K = 4 neighbours picked by src_index from a pool of 16 resident sensor maps
      b   8 views x 384 x 512, K = 7 sources given as [B, K, H, W]
Sources lie within 0.15 m / 0.06 rad of their view and see the same kind of surface, 10 % holes in every sensor map; the share
of pixel-source pairs that enter the loss is reported.  Fused and eager windows alternate inside one session; the median window
and the spread (min, max) of the per-call times are reported, with the four library calls alone (device events around
back-to-back calls on preallocated buffers), the bytes each form holds between forward and backward
(torch.cuda.memory_allocated after the forward minus before it), and the library calls as a share of the copy rate MEASURED IN
THIS SESSION (a 1 GiB device-to-device copy, read + written bytes over time) against the algorithmic byte floor: (3 + K) maps
read forward, (3 + K) maps read plus 2 maps written backward; 3 read, and 3 read plus 2 written, for the scale-invariant term.

Prints one JSON object and writes it to --out.    python bench_mv_depth.py [--reps 7 --warmup 3 --out profiles/mv_depth_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch

WORKLOADS = {"a": dict(B=4, H=968, W=1296, K=4, pool=16), "b": dict(B=8, H=384, W=512, K=7, pool=0)}


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
    out = forward()
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - before
    del out
    return int(held)


def copy_rate(dev, reps=5):
    """Bytes read + written per second of a 1 GiB device-to-device copy (beyond the 256 MiB last-level cache)."""
    src = torch.empty(1 << 28, device=dev).normal_()
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    torch.cuda.synchronize()
    ms = sorted(window_ms(lambda: dst.copy_(src), 10) for _ in range(reps))[reps // 2]
    return 2.0 * src.numel() * 4 / (1e-3 * ms)


def make_inputs(B, H, W, K, pool, dev):
    import mv_depth_cases as C
    from freesplat_amd import mv_depth_loss as M
    g = torch.Generator(device=dev).manual_seed(H + B)
    cpu = torch.Generator().manual_seed(H + B)
    y = torch.arange(H, device=dev).view(1, H, 1) / H
    x = torch.arange(W, device=dev).view(1, 1, W) / W

    def surface(n):
        ph = torch.rand(n, 4, 1, 1, device=dev, generator=g)
        return 2.4 + 0.5 * torch.sin(5.0 * x + 6.0 * ph[:, 0]) * torch.cos(4.0 * y + 6.0 * ph[:, 1]) + 0.3 * torch.sin(3.0 * (x + y) + 6.0 * ph[:, 2])

    def with_holes(t):
        return torch.where(torch.rand(t.shape, device=dev, generator=g) < 0.1, torch.full_like(t, float("nan")), t)

    clean = surface(B)
    gt = with_holes(clean)
    alpha = 0.3 + 0.7 * torch.rand(B, H, W, device=dev, generator=g)
    depth = clean * torch.exp(0.03 * torch.randn(B, H, W, device=dev, generator=g)) * alpha
    c2w = torch.stack([C.pose(cpu, 2.0, 0.5) for _ in range(B)])
    intr = C.intrinsics(H, W)
    n_src = pool if pool else B * K
    if pool:                                             # view b's neighbours are the pool maps b, b + B, b + 2 B, ...
        index = torch.tensor([[b + B * k for k in range(K)] for b in range(B)], dtype=torch.int32)
        owner = [i % B for i in range(pool)]
    else:
        index, owner = None, [i // K for i in range(n_src)]
    w2s = torch.stack([torch.linalg.inv(c2w[owner[i]] @ C.pose(cpu, 0.15, 0.06)) for i in range(n_src)])
    # a neighbour sees the same kind of surface, a little deeper on average: about two thirds of the points are not occluded
    src = with_holes(surface(n_src) * (1.0 + 0.05 * torch.rand(n_src, 1, 1, device=dev, generator=g)))
    if not pool:
        src, w2s = src.view(B, K, H, W), w2s.view(B, K, 4, 4)
    index = None if index is None else index.to(dev)
    pairs = M.pair_transforms(intr, c2w.to(dev), intr, w2s.to(dev), index)
    return dict(depth=depth, gt=gt, alpha=alpha, src=src, pairs=pairs, index=index)


def library_calls_us(t, K, S_pool, calls=30, reps=5):
    """Microseconds per call of the four entry points on preallocated buffers."""
    from freesplat_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    depth, gt, alpha, src, pairs, index = (t[k] for k in ("depth", "gt", "alpha", "src", "pairs", "index"))
    B, H, W = depth.shape
    dev = depth.device
    scratch = torch.empty(L.fs_mvdepth_scratch_bytes(B, K, H, W), dtype=torch.uint8, device=dev)
    total, cnt = torch.empty(2, B, K, dtype=torch.float64, device=dev)
    s1, s2, n = torch.empty(3, B, dtype=torch.float64, device=dev)
    g_sum, g_s = torch.ones(B, K, device=dev), torch.ones(B, device=dev)
    g_depth, g_alpha = torch.empty_like(depth), torch.empty_like(depth)
    st, mv, si = _lib.current_stream(), (1.05, 0.0, float("inf"), 1e-3), (0.0, float("inf"), 1e-3)
    sizes = (B, K, H, W, H, W, S_pool)
    fns = {
        "mv_fwd": lambda: _lib.check(L.fs_mv_depth_forward(*sizes, p(depth), p(gt), p(alpha), p(src), p(index), p(pairs), *mv, p(total),
                                                           p(cnt), None, p(scratch), st), "fs_mv_depth_forward"),
        "mv_bwd": lambda: _lib.check(L.fs_mv_depth_backward(*sizes, p(depth), p(gt), p(alpha), p(src), p(index), p(pairs), *mv, p(g_sum),
                                                            p(g_depth), p(g_alpha), st), "fs_mv_depth_backward"),
        "si_fwd": lambda: _lib.check(L.fs_si_depth_forward(B, H, W, p(depth), p(gt), p(alpha), *si, p(s1), p(s2), p(n), p(scratch), st),
                                     "fs_si_depth_forward"),
        "si_bwd": lambda: _lib.check(L.fs_si_depth_backward(B, H, W, p(depth), p(gt), p(alpha), *si, p(g_s), p(g_s), p(g_depth),
                                                            p(g_alpha), st), "fs_si_depth_backward"),
    }
    out = {}
    for name, fn in fns.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        out[name] = round(1e3 * sorted(window_ms(fn, calls) for _ in range(reps))[reps // 2], 1)
    return out


def make_case(name, dev):
    import mv_depth_ref as R
    from freesplat_amd import mv_depth_loss as M
    w = WORKLOADS[name]
    t = make_inputs(w["B"], w["H"], w["W"], w["K"], w["pool"], dev)
    depth, alpha = t["depth"].requires_grad_(True), t["alpha"].requires_grad_(True)
    gt, src, pairs, index = t["gt"], t["src"], t["pairs"], t["index"]
    leaves = [depth, alpha]
    mv_f = lambda: M.mv_depth_loss(depth, gt, src, pairs, alpha, src_index=index)
    mv_e = lambda: R.mv_depth_loss(depth, gt, src, pairs, alpha, src_index=index)
    si_f = lambda: M.scale_invariant_loss(depth, gt, alpha)
    si_e = lambda: R.scale_invariant_loss(depth, gt, alpha)

    def no_grad(fn):
        def run():
            with torch.no_grad():
                return fn()
        return run
    train = lambda fn: (lambda: torch.autograd.grad(fn(), leaves))
    fns = {}
    for term, fused, eager in (("mv", mv_f, mv_e), ("si", si_f, si_e)):
        fns.update({f"{term}_fused_fwd": no_grad(fused), f"{term}_eager_fwd": no_grad(eager),
                    f"{term}_fused_fwd_bwd": train(fused), f"{term}_eager_fwd_bwd": train(eager)})
    held = {"mv_fused": mv_f, "mv_eager": mv_e, "si_fused": si_f, "si_eager": si_e}
    selected = lambda: M.mv_depth_terms(depth.detach(), gt, src, pairs, alpha.detach(), src_index=index)[1].sum() / (w["B"] * w["K"] * w["H"] * w["W"])
    lib = lambda: library_calls_us({**t, "depth": depth.detach(), "alpha": alpha.detach()}, w["K"], w["pool"])
    counts = {"fused": lambda: M.mv_depth_terms(depth.detach(), gt, src, pairs, alpha.detach(), src_index=index)[1].sum(),
              "eager": lambda: R.terms(depth.detach(), gt, src, pairs, alpha.detach(), src_index=index)[1].sum()}
    return fns, held, selected, lib, counts


def report(name, case, reps, rate):
    fns, held, selected, lib, counts = case
    w = WORKLOADS[name]
    calls = {k: (30 if "fused" in k else 3) for k in fns}
    t = alternate(fns, calls, reps)
    lib_us = lib()
    map_bytes = 4 * w["B"] * w["H"] * w["W"]
    floor = {"mv_fwd": (3 + w["K"]) * map_bytes, "mv_bwd": (3 + w["K"] + 2) * map_bytes, "si_fwd": 3 * map_bytes, "si_bwd": 5 * map_bytes}
    row = {"workload": name, "views": w["B"], "H": w["H"], "W": w["W"], "K": w["K"], "pool": w["pool"], "alpha": True,
           "pairs_in_the_loss": round(float(selected()), 3), **t}
    for term in ("mv", "si"):
        lf, le = float(fns[f"{term}_fused_fwd"]()), float(fns[f"{term}_eager_fwd"]())
        gf, ge = fns[f"{term}_fused_fwd_bwd"](), fns[f"{term}_eager_fwd_bwd"]()
        row[term] = {
            "fwd_speedup": round(t[f"{term}_eager_fwd"]["median_ms"] / t[f"{term}_fused_fwd"]["median_ms"], 2),
            "fwd_bwd_speedup": round(t[f"{term}_eager_fwd_bwd"]["median_ms"] / t[f"{term}_fused_fwd_bwd"]["median_ms"], 2),
            "held_for_backward_bytes": {"fused": held_bytes(held[f"{term}_fused"]), "eager": held_bytes(held[f"{term}_eager"])},
            # the library calls alone, without the autograd wrapper and the torch glue: events around 30 back-to-back calls
            # (2 launches forward, 1 backward), i.e. the larger of their device time and their enqueue time
            "library_call_us": {"fwd": lib_us[f"{term}_fwd"], "bwd": lib_us[f"{term}_bwd"]},
            "algorithmic_floor_bytes": {"fwd": floor[f"{term}_fwd"], "bwd": floor[f"{term}_bwd"]},
            "library_call_share_of_copy_rate": {d: round(floor[f"{term}_{d}"] / rate / (1e-6 * lib_us[f"{term}_{d}"]), 3) for d in ("fwd", "bwd")},
            # the inputs are not made decidable: a pixel whose nearest source pixel or occlusion test falls the other way in the
            # eager fp32 chain carries a different gradient altogether, so the pixels beyond 1e-4 of max-abs are counted too
            "parity": {"loss_fused": lf, "loss_eager": le,
                       "grad_rel_diff_vs_eager": max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(gf, ge)),
                       "grad_pixels_beyond_1e-4_of_max": max(int(((a - b).abs() > 1e-4 * b.abs().max()).sum()) for a, b in zip(gf, ge))},
        }
    row["mv"]["parity"]["selected_pairs"] = {k: int(v()) for k, v in counts.items()}
    note(json.dumps(row))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mv_depth_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mv_depth.py needs a HIP device (no CPU fallback)")
    dev = torch.device("cuda:0")
    rate = copy_rate(dev)
    out = {"bench": "mv_depth", "device": torch.cuda.get_device_name(0), "baseline": "eager fp32 torch restatement "
           "(tests/mv_depth_ref.py under autograd) on the same device, same session, alternated windows",
           "copy_bytes_per_s_this_session": round(rate, -9), "reps": args.reps, "warmup": args.warmup, "rows": []}
    for name in WORKLOADS:                               # every shape is warmed before the first timed window
        fns = make_case(name, dev)[0]
        for fn in fns.values():
            for _ in range(args.warmup):
                fn()
        del fns
    torch.cuda.synchronize()
    for name in WORKLOADS:
        case = make_case(name, dev)
        for fn in case[0].values():
            fn()
        torch.cuda.synchronize()
        out["rows"].append(report(name, case, args.reps, rate))
        del case
        torch.cuda.empty_cache()
    out["fused_never_slower"] = all(r[t][k] >= 1.0 for r in out["rows"] for t in ("mv", "si") for k in ("fwd_speedup", "fwd_bwd_speedup"))
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
