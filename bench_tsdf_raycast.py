#!/usr/bin/env python
"""TSDF ray-casting benchmark (standalone; not the headline metric).  One process, everything warmed first.

Workload: the 256^3 colour volume of bench_tsdf.py (a sphere in front of a far wall, fused from 16 views of 968 x 1296 on a
ring), ray cast into 4 views of 968 x 1296 from cameras on the same ring BETWEEN the fused ones; --small: 128^3, 4 fused views
of 384 x 512, 2 ray-cast views of 384 x 512.

  library_*        fs_tsdf_raycast alone on prepared device arrays: depth only; depth + normals; depth + normals + colour + steps
  wrapper          TSDFVolume.raycast (argument checks, the camera rows, four allocations, one library call)
  eager_float32    the same march as a user writes it in fp32 torch: every ray in one masked loop, a sample = sixteen
                   advanced-indexing gathers, regula falsi and the final depth (no normals, no colour).  A yardstick, not code
                   under test; its depth is compared with the fused one
  copy             dst.copy_(src) of the full output's bytes (depth, normals, colour, steps)

The windows alternate inside one session; the median window and the spread (min, max) of the per-call times are reported, with
the samples the rays took (march samples + refinement samples + the final one per hit; mean and maximum march samples per ray,
the hit share) and each configuration's time per (ray, sample).  `resident_lane_ns_per_sample` is that time multiplied by the
lanes the chip holds at the kernel's occupancy (256 CUs x 32 wavefronts x 64 lanes): what one resident lane spends on a sample
if every lane slot were busy -- a few hundred ns is a memory round trip (latency binds), far more means idle lanes (divergence,
the tail of long rays), far less would mean the issue rate or bytes bind.

Prints one JSON object and writes it to --out.    python bench_tsdf_raycast.py [--reps 5 --out profiles/tsdf_raycast_bench.json]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch

from bench_tsdf import alternate, note, scene

RESIDENT_LANES = 256 * 32 * 64
REFINE = 4


def between_cameras(n_fused, n_cast):
    """Camera-to-world [n_cast, 4, 4] float64 on bench_tsdf.scene's ring, half a step after every (n_fused / n_cast)-th fused one."""
    c2w = torch.zeros(n_cast, 4, 4, dtype=torch.float64)
    for i in range(n_cast):
        th = 2 * math.pi * (i * (n_fused // n_cast) + 0.5) / n_fused
        pos = torch.tensor([2.0 * math.cos(th), 0.25 * math.sin(3 * th), 2.0 * math.sin(th)], dtype=torch.float64)
        z = -pos / pos.norm()
        x = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), z)
        x = x / x.norm()
        c2w[i, :3, 0], c2w[i, :3, 1], c2w[i, :3, 2], c2w[i, :3, 3], c2w[i, 3, 3] = x, torch.linalg.cross(z, x), z, pos, 1.0
    return c2w


def eager_raycast(vol, rows, k, H, W, step_min=0.5, relax=0.8, refine=REFINE, min_weight=1.0):
    """depth [V, H, W] by the header's march in fp32 torch (associations not pinned; no normals, no colour)."""
    X, Y, Z = vol.dims
    dev = vol.tsdf.device
    V = rows.shape[0]
    f, w = vol.tsdf.reshape(-1), vol.weight.reshape(-1)
    py, px = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    dxy = torch.stack([(px[None] - k[:, 2, None, None]) / k[:, 0, None, None], (py[None] - k[:, 3, None, None]) / k[:, 1, None, None],
                       torch.ones(V, H, W, device=dev)], -1).reshape(V, -1, 3)
    org = torch.tensor(vol.origin, device=dev)
    o = ((rows[:, :, 3] - org) / vol.voxel_size)[:, None, :].expand(V, H * W, 3).reshape(-1, 3)
    d = (dxy @ rows[:, :, :3].transpose(1, 2) / vol.voxel_size).reshape(-1, 3)
    n1 = torch.tensor([X - 1.0, Y - 1.0, Z - 1.0], device=dev)
    lo, hi = (0.0 - o) / d, (n1 - o) / d
    s0 = torch.minimum(lo, hi).nan_to_num(nan=-math.inf).amax(1).clamp_min(0.0)
    s1 = torch.maximum(lo, hi).nan_to_num(nan=math.inf).amin(1)
    L = d.norm(dim=1)
    tv = vol.trunc / vol.voxel_size
    offs = torch.tensor([(q & 1) + ((q >> 1) & 1) * X + ((q >> 2) & 1) * X * Y for q in range(8)], device=dev)
    nm2 = n1 - 1.0

    def sample(s):
        g = o + s[:, None] * d
        fi = torch.minimum(g.floor().clamp_min(0.0).nan_to_num(nan=0.0), nm2)
        t = g - fi
        i = fi.long()
        idx = ((i[:, 2] * Y + i[:, 1]) * X + i[:, 0])[:, None] + offs
        c, ww = f[idx], w[idx]
        c = c[:, 0::2] + t[:, 0:1] * (c[:, 1::2] - c[:, 0::2])
        c = c[:, 0::2] + t[:, 1:2] * (c[:, 1::2] - c[:, 0::2])
        return (ww >= min_weight).all(1), c[:, 0] + t[:, 2] * (c[:, 1] - c[:, 0])

    active = s0 <= s1
    s = s0.clone()
    sa, fa, sb, fb = (torch.zeros_like(s) for _ in range(4))
    prev = torch.zeros_like(active)
    hit = torch.zeros_like(active)
    for _ in range(4 * (X + Y + Z)):
        if not bool(active.any()):
            break
        obs, fv = sample(s)
        cross = active & prev & obs & ~(fa < 0) & (fv < 0)
        sb, fb = torch.where(cross, s, sb), torch.where(cross, fv, fb)
        hit |= cross
        go = active & ~cross
        sa, fa, prev = torch.where(go, s, sa), torch.where(go, fv, fa), torch.where(go, obs, prev)
        step = torch.where(obs, (relax * (fv.abs() * tv)).clamp_min(step_min).nan_to_num(nan=step_min), torch.full_like(s, relax * tv))
        s = torch.where(go, s + step / L, s)
        active = go & (s <= s1)
    for _ in range(refine):
        sm = sa + (fa / (fa - fb)) * (sb - sa)
        obs, fv = sample(sm)
        to_b, to_a = hit & obs & (fv < 0), hit & obs & ~(fv < 0)
        sb, fb = torch.where(to_b, sm, sb), torch.where(to_b, fv, fb)
        sa, fa = torch.where(to_a, sm, sa), torch.where(to_a, fv, fa)
    return torch.where(hit, sa + (fa / (fa - fb)) * (sb - sa), torch.zeros_like(s)).reshape(V, H, W)


def workload(name, n, V_fused, Hf, Wf, V, H, W, args, dev):
    from freesplat_amd import _lib
    from freesplat_amd.tsdf import TSDFVolume, cam_rows
    origin, vs, c2w_fused, intr, depth_in, image = scene(n, V_fused, Hf, Wf, dev)
    vol = TSDFVolume(origin, vs, (n, n, n), 4 * vs, color=True, max_weight=64.0, device=dev)
    vol.integrate(depth_in, intr, c2w_fused, image=image)
    del depth_in, image
    c2w = between_cameras(V_fused, V)
    rows = cam_rows(c2w, dev)
    fcast = 2.5 * W
    k = torch.tensor([fcast, fcast, (W - 1) / 2, (H - 1) / 2], device=dev).expand(V, 4).contiguous()
    max_steps = 4 * 3 * n
    depth, nrm, col = torch.empty(V, H, W, device=dev), torch.empty(V, 3, H, W, device=dev), torch.empty(V, 3, H, W, device=dev)
    steps = torch.empty(V, H, W, dtype=torch.int32, device=dev)
    L, p = _lib.lib(), _lib.ptr

    def library(normals, color, with_steps):
        def call():
            _lib.check(L.fs_tsdf_raycast(n, n, n, *vol.origin, vol.voxel_size, vol.trunc, p(vol.tsdf), p(vol.weight), p(vol.color), V, H, W,
                                         p(rows), p(k), 0.0, math.inf, 1.0, 0.5, 0.8, REFINE, max_steps, p(depth), p(nrm) if normals else None,
                                         p(col) if color else None, p(steps) if with_steps else None, _lib.current_stream()), "fs_tsdf_raycast")
        return call

    library(True, True, True)()
    rays = V * H * W
    hits = int((depth > 0).sum())
    march = int(steps.sum())
    samples = march + hits * (REFINE + 1)
    eager_depth = eager_raycast(vol, rows, k, H, W)
    same_hit = float(((eager_depth > 0) == (depth > 0)).float().mean())
    both = (eager_depth > 0) & (depth > 0)
    diff = float((eager_depth - depth)[both].abs().max() / vs)
    note(f"{name}: {100 * hits / rays:.1f} % of {rays} rays hit, {march / rays:.2f} march samples per ray (at most {int(steps.max())}), {samples} samples in "
         f"all; eager torch agrees on hit / no hit at {100 * same_hit:.3f} % of the rays, max |depth difference| on common hits {diff:.2e} voxels")

    out_bytes = 4 * rays * 8
    src = torch.empty(out_bytes // 4, device=dev).normal_()
    dst = torch.empty_like(src)
    fns = {"library_depth": library(False, False, False), "library_depth_normals": library(True, False, False),
           "library_all_outputs": library(True, True, True), "wrapper": lambda: vol.raycast(k, c2w, (H, W)),
           "copy": lambda: dst.copy_(src), "eager_float32": lambda: eager_raycast(vol, rows, k, H, W)}
    calls = {"default": args.calls, "eager_float32": 1}
    for fn in fns.values():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
    res = alternate(fns, calls, args.reps)
    for key in ("library_depth", "library_depth_normals", "library_all_outputs", "wrapper", "eager_float32"):
        ns = 1e6 * res[key]["median_ms"] / samples
        res[key]["ns_per_ray_sample"] = round(ns, 5)
        res[key]["resident_lane_ns_per_sample"] = round(ns * RESIDENT_LANES, 1)
    res["copy"]["GB_per_s_read_plus_written"] = round(2.0 * out_bytes / (1e-3 * res["copy"]["median_ms"]) / 1e9, 1)
    res["eager_float32"]["over_wrapper"] = round(res["eager_float32"]["median_ms"] / res["wrapper"]["median_ms"], 2)
    return {"grid": [n, n, n], "fused_views": V_fused, "views": V, "map": [H, W], "rays": rays, "hit_share": round(hits / rays, 4),
            "march_samples_per_ray_mean": round(march / rays, 3), "march_samples_per_ray_max": int(steps.max()), "samples": samples,
            "output_bytes": out_bytes, "eager_same_hit_share": round(same_hit, 6), "eager_max_depth_difference_voxels": diff, "windows": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_raycast_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf_raycast.py needs a HIP device (no CPU fallback)")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "calls_per_window": args.calls, "refine": REFINE,
              "resident_lanes_assumed": RESIDENT_LANES}
    if args.small:
        big = result["128_2x384x512"] = workload("128^3, 2 views of 384 x 512", 128, 4, 384, 512, 2, 384, 512, args, dev)
    else:
        big = result["256_4x968x1296"] = workload("256^3, 4 views of 968 x 1296", 256, 16, 968, 1296, 4, 968, 1296, args, dev)
    w = big["windows"]
    ms = lambda key: f"{w[key]['median_ms']:.2f} ms"
    result["readme"] = (
        f"{big['grid'][0]}^3 grid points with colour fused from {big['fused_views']} views, ray cast into {big['views']} views of {big['map'][0]} x "
        f"{big['map'][1]} ({result['device']}): {100 * big['hit_share']:.0f} % of the rays hit, {big['march_samples_per_ray_mean']:.1f} march samples per ray "
        f"(at most {big['march_samples_per_ray_max']}); fs_tsdf_raycast alone {ms('library_depth')} for depth, {ms('library_depth_normals')} with normals, "
        f"{ms('library_all_outputs')} with normals, colour and steps ({w['library_all_outputs']['ns_per_ray_sample'] * 1e3:.1f} ps per (ray, sample), "
        f"{w['library_all_outputs']['resident_lane_ns_per_sample']:.0f} ns per sample of a resident lane); TSDFVolume.raycast {ms('wrapper')}; a copy_ of the "
        f"output's bytes {ms('copy')}; the same march in eager fp32 torch {ms('eager_float32')} ({w['eager_float32']['over_wrapper']:.0f} x).")
    note(result["readme"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
