#!/usr/bin/env python
"""TSDF fusion and mesh extraction benchmark (standalone; not the headline metric).  One process, everything warmed first.

Workloads: 256^3 grid points with colour (5 planes: 336 MB, 671 MB read + written when every point is updated), 16 views of
968 x 1296; and 128^3 with 4 views of 384 x 512.  The cameras stand on a ring around the volume and look at a sphere in front of
a far wall, with a focal length that leaves roughly half of the grid inside some frustum (the measured share is reported).

  integrate        TSDFVolume.integrate (the Python wrapper: argument checks, the float64 inverse of the extrinsics, one
                   library call), and fs_tsdf_integrate alone on prepared device arrays -- with the brick-level view skip and
                   with FS_TSDF_NO_BRICK_SKIP (the A/B of the skip, inside this session)
  extract          extract_mesh as a whole, and fs_tsdf_mesh_plan, the read-back of the total and fs_tsdf_mesh_emit separately
  eager            the same integration as a user writes it in fp32 torch: per view a projection of all grid points, an index
                   gather and masked updates.  A yardstick, not code under test; its result is compared with the fused one
  copy             dst.copy_(src) of the volume's bytes (reads them and writes as many): the rate ceiling of this session

The windows alternate inside one session; the median window and the spread (min, max) of the per-call times are reported, the
fused call's grid-point-views per second, its bytes (the planes of the updated points, read + written, plus the maps) as a
share of the copy's rate, and its VALU work as a share of the issue rate (VALU_PER_PAIR instructions for each of the X Y Z V
(grid point, view) pairs -- an upper bound: skipped bricks walk fewer -- plus VALU_PER_UPDATE per update, counted in the
compiled kernel's loop; 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz).

Prints one JSON object and writes it to --out.    python bench_tsdf.py [--reps 5 --out profiles/tsdf_bench.json]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch

# the colour kernel compiles to 1056 v_* instructions, about 450 of them before and after the view loop; the loop body handles
# four grid points: about 60 per point up to the range test (two correctly rounded divisions), about 90 more for an update
# (sdf / trunc and the four running means: five divisions)
VALU_PER_PAIR, VALU_PER_UPDATE = 60, 90
VALU_LANE_OPS_PER_S = 256 * 4 * 16 * 2.4e9


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
    times = {k: [] for k in fns}
    for rep in range(reps):
        for k, fn in fns.items():
            times[k].append(window_ms(fn, calls.get(k, calls["default"])))
        note(f"round {rep + 1} of {reps}: " + ", ".join(f"{k} {v[-1]:.3f}" for k, v in times.items()))
    stat = lambda v: {"median_ms": round(sorted(v)[len(v) // 2], 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    return {k: stat(v) for k, v in times.items()}


def scene(n, V, H, W, dev):
    """(origin, voxel_size, c2w [V,4,4] float64 cpu, intrinsics [4], depth [V,H,W], image [V,3,H,W]): a unit cube of n^3 grid
    points, a sphere of radius 0.3 at its centre in front of a wall 3.2 from every camera, cameras on a ring of radius 2."""
    vs = 1.0 / (n - 1)
    origin = (-0.5, -0.5, -0.5)
    c2w = torch.zeros(V, 4, 4, dtype=torch.float64)
    for v in range(V):
        th = 2 * math.pi * v / V
        pos = torch.tensor([2.0 * math.cos(th), 0.25 * math.sin(3 * th), 2.0 * math.sin(th)], dtype=torch.float64)
        z = -pos / pos.norm()
        x = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), z)
        x = x / x.norm()
        c2w[v, :3, 0], c2w[v, :3, 1], c2w[v, :3, 2], c2w[v, :3, 3], c2w[v, 3, 3] = x, torch.linalg.cross(z, x), z, pos, 1.0
    f = 2.5 * W
    intr = torch.tensor([f, f, (W - 1) / 2, (H - 1) / 2])
    py, px = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    depth = torch.empty(V, H, W, device=dev)
    for v in range(V):
        E = c2w[v].to(dev)
        ray = torch.stack([(px - intr[2].item()) / f, (py - intr[3].item()) / f, torch.ones_like(px)], -1) @ E[:3, :3].T
        oc = E[:3, 3]
        a, b, c = (ray * ray).sum(-1), (ray * oc).sum(-1), float(oc @ oc) - 0.09
        disc = b * b - a * c
        depth[v] = torch.where(disc > 0, (-b - disc.clamp_min(0).sqrt()) / a, torch.full_like(a, 3.2)).float()
    image = torch.rand(V, 3, H, W, device=dev, generator=torch.Generator(dev).manual_seed(0))
    return origin, vs, c2w, intr, depth, image


def eager_integrate(state, pts, w2c, intr, depth, image, trunc, max_weight, near=1e-3):
    """One view after the other in fp32 torch: state = [tsdf, weight, c0, c1, c2] flat over the grid points."""
    tsdf, wgt = state[0], state[1]
    V, H, W = depth.shape
    for v in range(V):
        p = pts @ w2c[v, :, :3].T + w2c[v, :, 3]
        z = p[:, 2]
        ix = torch.round(intr[v, 0] * (p[:, 0] / z) + intr[v, 2])
        iy = torch.round(intr[v, 1] * (p[:, 1] / z) + intr[v, 3])
        ok = (z > near) & (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        pix = torch.where(ok, iy * W + ix, torch.zeros_like(ix)).long()
        d = depth[v].reshape(-1)[pix]
        sdf = d - z
        ok = ok & torch.isfinite(d) & (d > 0) & ~(sdf < -trunc)
        s = torch.clamp(sdf / trunc, max=1.0)
        w1 = wgt + 1.0
        tsdf.copy_(torch.where(ok, (tsdf * wgt + s) / w1, tsdf))
        for ch in range(3):
            c = image[v, ch].reshape(-1)[pix]
            state[2 + ch].copy_(torch.where(ok, (state[2 + ch] * wgt + c) / w1, state[2 + ch]))
        wgt.copy_(torch.where(ok, torch.clamp(w1, max=max_weight), wgt))


def workload(name, n, V, H, W, args, dev):
    from freesplat_amd import _lib
    from freesplat_amd.tsdf import TSDFVolume, extract_mesh, world_to_cam
    origin, vs, c2w, intr, depth, image = scene(n, V, H, W, dev)
    trunc = 4 * vs
    vol = TSDFVolume(origin, vs, (n, n, n), trunc, color=True, max_weight=64.0, device=dev)
    w2c = world_to_cam(c2w, dev)
    k = intr.to(dev).expand(V, 4).contiguous()
    L, p = _lib.lib(), _lib.ptr
    kw = dict(near=1e-3, min_depth=0.0, max_depth=math.inf, alpha_min=0.5, alpha_floor=1e-3)

    def library(flags):
        def call():
            _lib.check(L.fs_tsdf_integrate(n, n, n, *vol.origin, vol.voxel_size, vol.trunc, vol.max_weight, p(vol.tsdf), p(vol.weight),
                                           p(vol.color), V, H, W, p(w2c), p(k), p(depth), None, p(image), 1e-3, 0.0, math.inf, 0.5, 1e-3,
                                           flags, _lib.current_stream()), "fs_tsdf_integrate")
        return call

    # ---- what one call fuses, and the eager form's agreement with it
    vol.integrate(depth, intr, c2w, image=image, **kw)
    updates = float(vol.weight.sum())                                       # (weights count updates: max_weight is not reached)
    inside = float((vol.weight > 0).sum()) / n ** 3
    pts = vol.grid_points().reshape(-1, 3)
    state = [torch.ones(n ** 3, device=dev), torch.zeros(n ** 3, device=dev)] + [torch.zeros(n ** 3, device=dev) for _ in range(3)]
    eager_integrate(state, pts, w2c, k, depth, image, vol.trunc, vol.max_weight)
    same_w = float((state[1] == vol.weight.reshape(-1)).float().mean())
    agree = state[1] == vol.weight.reshape(-1)
    diff = float((state[0] - vol.tsdf.reshape(-1))[agree].abs().max())
    note(f"{name}: {100 * inside:.1f} % of the grid inside some frustum and updated, {updates / n ** 3:.2f} updates per grid point; eager "
         f"torch gives the same weight at {100 * same_w:.3f} % of the points, max |tsdf difference| there {diff:.2e}")

    src = torch.empty(5 * n ** 3, device=dev).normal_()
    dst = torch.empty_like(src)
    scratch = torch.empty(L.fs_tsdf_mesh_scratch_bytes(n, n, n), dtype=torch.uint8, device=dev)
    total = torch.empty(1, dtype=torch.int64, device=dev)

    def plan():
        _lib.check(L.fs_tsdf_mesh_plan(n, n, n, p(vol.tsdf), p(vol.weight), 1.0, p(total), p(scratch), _lib.current_stream()), "fs_tsdf_mesh_plan")

    plan()
    T = int(total.item())
    verts, cols = torch.empty(T, 3, 3, device=dev), torch.empty(T, 3, 3, device=dev)

    def emit():
        _lib.check(L.fs_tsdf_mesh_emit(n, n, n, *vol.origin, vol.voxel_size, p(vol.tsdf), p(vol.weight), p(vol.color), 1.0, p(scratch), T,
                                       p(verts), p(cols), _lib.current_stream()), "fs_tsdf_mesh_emit")

    def eager():
        for s, init in zip(state, (1.0, 0.0, 0.0, 0.0, 0.0)):
            s.fill_(init)
        eager_integrate(state, pts, w2c, k, depth, image, vol.trunc, vol.max_weight)

    def fresh(fn):                                                          # every call fuses into an empty volume, like the first
        def call():
            vol.reset()
            fn()
        return call

    fns = {"reset": vol.reset, "integrate_wrapper": fresh(lambda: vol.integrate(depth, intr, c2w, image=image, **kw)),
           "integrate_library": fresh(library(0)), "integrate_library_no_brick_skip": fresh(library(_lib.TSDF_NO_BRICK_SKIP)),
           "copy": lambda: dst.copy_(src), "eager_float32": eager}
    calls = {"default": args.calls, "eager_float32": max(1, args.calls // 5)}
    for key, fn in fns.items():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
    res = alternate(fns, calls, args.reps)
    # the extraction reads the fused volume: integrate once more, then time its parts
    vol.reset()
    vol.integrate(depth, intr, c2w, image=image, **kw)
    mesh = {"extract_mesh": lambda: extract_mesh(vol.tsdf, vol.weight, vol.color, vol.origin, vol.voxel_size), "mesh_plan": plan,
            "mesh_total_read_back": lambda: total.item(), "mesh_emit": emit}
    for fn in mesh.values():
        fn()
    torch.cuda.synchronize()
    res.update(alternate(mesh, {"default": args.calls}, args.reps))

    plane_bytes = 5 * 4 * n ** 3
    copy_rate = 2.0 * plane_bytes / (1e-3 * res["copy"]["median_ms"])
    res["copy"]["GB_per_s_read_plus_written"] = round(copy_rate / 1e9, 1)
    for key in ("integrate_library", "integrate_library_no_brick_skip", "integrate_wrapper"):
        ms = res[key]["median_ms"] - res["reset"]["median_ms"]
        res[key]["median_ms_without_reset"] = round(ms, 4)
        moved = 2.0 * plane_bytes * inside + 4.0 * 4 * V * H * W
        res[key]["share_of_copy_rate"] = round(moved / (1e-3 * ms) / copy_rate, 3)
        res[key]["point_views_per_s"] = round(updates / (1e-3 * ms), 1)
        valu = VALU_PER_PAIR * float(V) * n ** 3 + VALU_PER_UPDATE * updates
        res[key]["share_of_valu_issue_rate"] = round(valu / (1e-3 * ms) / VALU_LANE_OPS_PER_S, 3)
    res["eager_float32"]["over_integrate_wrapper"] = round(res["eager_float32"]["median_ms"] / res["integrate_wrapper"]["median_ms"], 2)
    return {"grid": [n, n, n], "views": V, "map": [H, W], "volume_bytes": plane_bytes, "share_of_grid_updated": round(inside, 4),
            "updates_per_grid_point": round(updates / n ** 3, 3), "triangles": T, "eager_same_weight_share": round(same_w, 6),
            "eager_max_tsdf_difference": diff, "windows": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--small-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tsdf.py needs a HIP device (no CPU fallback)")
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "calls_per_window": args.calls,
              "valu_per_pair_assumed": VALU_PER_PAIR, "valu_per_update_assumed": VALU_PER_UPDATE}
    result["128_4x384x512"] = workload("128^3, 4 views of 384 x 512", 128, 4, 384, 512, args, dev)
    if not args.small_only:
        result["256_16x968x1296"] = workload("256^3, 16 views of 968 x 1296", 256, 16, 968, 1296, args, dev)
    big = result.get("256_16x968x1296", result["128_4x384x512"])
    w = big["windows"]
    ms = lambda key: f"{w[key]['median_ms']:.2f} ms"
    result["readme"] = (
        f"{big['grid'][0]}^3 grid points with colour, {big['views']} views of {big['map'][0]} x {big['map'][1]} ({result['device']}), "
        f"{100 * big['share_of_grid_updated']:.0f} % of the grid updated: TSDFVolume.integrate {w['integrate_wrapper']['median_ms_without_reset']:.2f} ms, "
        f"fs_tsdf_integrate alone {w['integrate_library']['median_ms_without_reset']:.2f} ms "
        f"({100 * w['integrate_library']['share_of_copy_rate']:.0f} % of the rate of a copy_ of the volume's bytes, {ms('copy')}, "
        f"{w['copy']['GB_per_s_read_plus_written']:.0f} GB/s read + written; {100 * w['integrate_library']['share_of_valu_issue_rate']:.0f} % of "
        f"the VALU issue rate at {VALU_PER_PAIR} instructions per (grid point, view) pair and {VALU_PER_UPDATE} per update), without the brick-level view skip "
        f"{w['integrate_library_no_brick_skip']['median_ms_without_reset']:.2f} ms; the same integration in eager fp32 torch {ms('eager_float32')} "
        f"({w['eager_float32']['over_integrate_wrapper']:.1f} x); extract_mesh {ms('extract_mesh')} for {big['triangles']} triangles "
        f"(plan {ms('mesh_plan')}, read-back {ms('mesh_total_read_back')}, emit {ms('mesh_emit')}).")
    note(result["readme"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
