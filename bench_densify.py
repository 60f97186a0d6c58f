#!/usr/bin/env python
"""Gaussian density-control benchmark (standalone; not the headline metric): one densification of 1.0 M Gaussians at SH degree 3
(M = 16, 59 floats per Gaussian, parameters + exp_avg + exp_avg_sq), with about 10 % of the rows cloned, 10 % split and 5 %
dropped, drawn at random.  One process, everything warmed first.

  fused        freesplat_amd.refine.GaussianAdam.densify: fs_density_plan (three launches), the read of the four counters (the
               one host sync), the allocation of the new buffers, fs_density_apply (one launch), new statistics and leaves.
               Run on a shallow copy of the optimizer each time, so that every call starts from the same 1.0 M rows.
  fused_plan   the plan with its read-back alone; fused_apply: the fs_density_apply launch alone, into buffers allocated once.
  eager        the same operation as a user writes it in torch today: boolean masks from the statistics, `cat` of the surviving
               rows, the clones' copies and the split children over the five parameter arrays, zero-padded moments, eager
               exp / sigmoid for the activated leaves.  Children drawn with torch.randn.  A yardstick, not code under test.
ms per call INCLUDE the Python wrapper and, for `fused` and `eager`, the host synchronisation each contains: device events
around windows of back-to-back calls, the windows of the forms alternated inside one session; median and spread (min, max).
The byte floor is source rows read plus destination rows written over the measured 6.29 TB/s copy rate (bench_refine.py).

Acceptance: the fused call must not be slower than the eager form in this session's numbers; the process exits 1 otherwise.

Prints one JSON object and writes it to --out.    python bench_densify.py [--reps 7 --warmup 2 --out profiles/gaussian_densify_bench.json]
"""
import argparse
import copy
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch

N, M = 1_000_000, 16
HBM_BYTES_PER_S = 6.29e12          # measured float4 copy rate (bench_refine.py, DESIGN.md "Evaluation metrics")
FLOATS = 3 + 3 + 4 + 1 + 3 * M     # per Gaussian
GRAD_T, DENSE, MIN_OP = 2e-4, 0.03, 0.005


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--gaussians", type=int, default=N)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gaussian_densify_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_densify.py needs a HIP device (no CPU fallback)")
    from freesplat_amd import _lib
    from freesplat_amd.refine import GaussianAdam
    dev = torch.device("cuda:0")
    n = args.gaussians
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)
    u = torch.rand(n, device=dev, generator=gen)
    clone, split, drop = u < 0.10, (u >= 0.10) & (u < 0.20), (u >= 0.20) & (u < 0.25)
    log_scales = torch.where(split[:, None], -2.0 + 0.3 * rnd(n, 3), -5.0 + 0.3 * rnd(n, 3))     # 0.135 / 0.007 around DENSE = 0.03
    logits = torch.where(drop, torch.full((n,), -7.0, device=dev), rnd(n).clamp(-3.0, 6.0))
    opt = GaussianAdam(rnd(n, 3), torch.exp(log_scales), rnd(n, 4), torch.sigmoid(logits), 0.3 * rnd(n, M, 3), sparse=True)
    sd = opt.state_dict()
    for k in ("means", "log_scales", "rotations", "logits", "shs"):
        sd["exp_avg." + k] = 1e-3 * rnd(*sd[k].shape)
        sd["exp_avg_sq." + k] = 1e-6 * torch.rand(sd[k].shape, device=dev, generator=gen)
    sd["density.denom"] = torch.randint(1, 4, (n,), device=dev, generator=gen).float()
    sd["density.grad_accum"] = sd["density.denom"] * torch.where(clone | split, 3.0 * GRAD_T, 0.3 * GRAD_T)
    sd["density.max_radii"] = torch.randint(1, 40, (n,), device=dev, generator=gen).float()
    opt.load_state_dict(sd)
    kw = dict(extent=1.0, grad_threshold=GRAD_T, min_opacity=MIN_OP, percent_dense=DENSE, seed=0)
    th = [GRAD_T, DENSE, MIN_OP, 0.0, 0.0, 0.0]

    # ---- fused
    info = {}

    def fused():
        info.update(copy.copy(opt).densify(**kw))

    fused()
    torch.cuda.synchronize()
    assert opt.N == n and info["n_out"] != n, info
    n_out = info["n_out"]

    def fused_plan():
        opt._plan(th)

    _, _, src, _ = opt._plan(th)
    new = [[torch.empty((n_out,) + tuple(t.shape[1:]), device=dev) for t in opt._raw] for _ in range(3)]
    out_s, out_o = torch.empty(n_out, 3, device=dev), torch.empty(n_out, 1, device=dev)
    tab = lambda ts: (C.c_void_p * 5)(*[t.data_ptr() for t in ts])
    dst_tables = [tab(ts) for ts in new]
    L, p = _lib.lib(), _lib.ptr

    def fused_apply():
        _lib.check(L.fs_density_apply(n, M, n_out, p(src), *opt._tables, *dst_tables, p(out_s), p(out_o), 0,
                                      _lib.current_stream()), "fs_density_apply")

    # ---- eager: masks, cat, index copies over parameters and both moments
    raw, m1, m2 = opt._raw, opt.exp_avg, opt.exp_avg_sq
    keep_result = {}

    @torch.no_grad()
    def eager():
        hot = (opt.denom > 0) & (opt.grad_accum >= GRAD_T * opt.denom)
        s_max = opt._scales.max(1).values
        is_split = hot & (s_max > DENSE)
        dropped = opt._opacities.reshape(-1) < MIN_OP
        stay, cl, sp = ~dropped & ~is_split, hot & ~is_split & ~dropped, is_split & ~dropped
        q = raw[2][sp]
        q = q / q.norm(dim=1, keepdim=True)
        r, x, y, z = q.unbind(-1)
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                         2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                         2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3).repeat(2, 1, 1)
        s = torch.exp(raw[1][sp]).repeat(2, 1)
        out_p, out_m, out_v = [], [], []
        for k in range(5):
            children = raw[k][sp].repeat((2,) + (1,) * (raw[k].dim() - 1))
            if k == 0:
                children = children + torch.bmm(R, (s * torch.randn_like(s)).unsqueeze(-1)).squeeze(-1)
            if k == 1:
                children = children - math.log(1.6)
            new_rows = torch.cat([raw[k][cl], children])
            out_p.append(torch.cat([raw[k][stay], new_rows]))
            pad = torch.zeros_like(new_rows)
            out_m.append(torch.cat([m1[k][stay], pad]))
            out_v.append(torch.cat([m2[k][stay], pad]))
        total = out_p[0].shape[0]
        keep_result["n_out"] = total
        keep_result["state"] = (out_p, out_m, out_v, torch.exp(out_p[1]), torch.sigmoid(out_p[3]).reshape(-1, 1),
                                torch.zeros(total, device=dev), torch.zeros(total, device=dev), torch.zeros(total, device=dev),
                                torch.zeros(total, 3, device=dev))

    eager()
    torch.cuda.synchronize()
    assert keep_result["n_out"] == n_out, (keep_result["n_out"], n_out)

    fns = {"fused": fused, "fused_plan": fused_plan, "fused_apply": fused_apply, "eager": eager}
    calls = {"fused": 20, "fused_plan": 50, "fused_apply": 100, "eager": 10}
    t = alternate(fns, calls, args.reps, args.warmup)

    rows_read_p = n - info["n_dropped"]
    rows_read_mv = n - info["n_dropped"] - info["n_split"]
    apply_bytes = 4 * FLOATS * (rows_read_p + 2 * rows_read_mv + 3 * n_out) + 16 * n_out + 4 * n_out      # + activated values written, src read
    floor_ms = 1e3 * apply_bytes / HBM_BYTES_PER_S
    rows = {k: dict(v, calls_per_window=calls[k]) for k, v in t.items()}
    rows["fused_apply"].update(algorithmic_bytes=apply_bytes,
                               share_of_measured_copy_rate=round(floor_ms / rows["fused_apply"]["median_ms"], 3))
    for k, v in rows.items():
        note(f"{k}: {json.dumps(v)}")
    ok = rows["fused"]["median_ms"] <= rows["eager"]["median_ms"]
    out = {"bench": "gaussian_densify", "device": torch.cuda.get_device_name(0), "gaussians": n, "sh_coefficients": M,
           "floats_per_gaussian": FLOATS, "counts": info, "hbm_bytes_per_s": HBM_BYTES_PER_S, "reps": args.reps, "warmup": args.warmup,
           "timing": "ms per call including the Python wrapper (and the host synchronisation inside fused, fused_plan and eager); "
                     "device events around windows of back-to-back calls, windows of the forms alternated; median (min, max)",
           "apply_byte_floor_ms": round(floor_ms, 4), "rows": rows,
           "acceptance": {"fused_median_ms": rows["fused"]["median_ms"], "eager_median_ms": rows["eager"]["median_ms"],
                          "fused_not_slower_than_eager": bool(ok)},
           "speedup_of_fused_over_eager": round(rows["eager"]["median_ms"] / rows["fused"]["median_ms"], 2)}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)
    if not ok:
        raise SystemExit("bench_densify.py: the fused densify is slower than the eager torch form in this session")


if __name__ == "__main__":
    main()
