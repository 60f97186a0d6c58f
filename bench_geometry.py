#!/usr/bin/env python
"""Geometry-metrics benchmark (standalone; not the headline metric).  One process, everything warmed first.

Workload: the sphere scene of bench_tsdf.py fused into a 128^3 volume from 8 views of 384 x 512, extracted, welded and sampled to
N points (sample_mesh), against N analytic points on the same sphere; N = 200 000 (the usual protocol size) and 1 000 000.

  grid_build          NearestGrid(gt): bounds (the one host read), keys, stable sort, gather, cell starts
  library             fs_nn_query alone on prepared device arrays, queries in their own (random) order, dist2 + index
  library_cell_order  the same with a prepared permutation of the queries by their own cell (the sort is not in the window)
  nearest             nearest(pred, grid) as called: query keys + sort + the launch + sqrt (cell order from SORT_QUERIES_FROM queries on)
  nearest_unsorted    nearest(pred, grid, sort_queries=False)
  geometry_metrics    geometry_metrics(pred, gt): two grid builds, two queries with their sums, the scalars
  cdist               the baseline: the same nearest distances by chunked torch.cdist(...).min(1), same device, same session
  copy                dst.copy_(src) of 256 MiB: the session's copy rate

The windows alternate inside one session; the median window and the spread (min, max) of the per-call times are reported.
`visited` is the number of reference points a query looked at (mean, max over 2000 of the queries), counted by the restatement
tests/geometry_ref.py of the same search on the same grid -- the product kernel has no counting path.

Prints one JSON object and writes it to --out.    python bench_geometry.py [--reps 5 --out profiles/geometry_metrics_bench.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from bench_tsdf import alternate, note, scene

RADIUS = 0.3      # bench_tsdf.scene's sphere, centred at the origin


def mesh(dev, n=128, V=8, H=384, W=512):
    from freesplat_amd.tsdf import TSDFVolume, weld
    origin, vs, c2w, intr, depth, image = scene(n, V, H, W, dev)
    vol = TSDFVolume(origin, vs, (n, n, n), 4 * vs, color=False, device=dev)
    vol.integrate(depth, intr, c2w)
    verts, faces, _ = weld(vol.extract_mesh()[0])
    return verts, faces, vs


def sphere_points(n, dev, seed):
    v = torch.randn(n, 3, dtype=torch.float64, device=dev, generator=torch.Generator(dev).manual_seed(seed))
    return (RADIUS * v / v.norm(dim=1, keepdim=True)).float()


def cdist_nearest(q, r, chunk):
    out = torch.empty(q.shape[0], device=q.device)
    for s in range(0, q.shape[0], chunk):
        out[s: s + chunk] = torch.cdist(q[s: s + chunk], r).min(1).values
    return out


def workload(N, verts, faces, vs, args, dev):
    import geometry_ref as G
    from freesplat_amd import _lib
    from freesplat_amd.geometry_metrics import NearestGrid, geometry_metrics, nearest, sample_mesh
    pred = sample_mesh(verts, faces, N, seed=0)
    gt = sphere_points(N, dev, 1)
    grid = NearestGrid(gt)
    keys = torch.empty(N, dtype=torch.int32, device=dev)
    p = _lib.ptr
    _lib.launch("fs_nn_grid_keys", N, p(pred), *grid._grid_args(), p(keys))
    order = torch.sort(keys, stable=True).indices
    dist2, index = torch.empty(N, device=dev), torch.empty(N, dtype=torch.int32, device=dev)
    L, tau = _lib.lib(), (C.c_float * 1)()

    def library(perm):
        def call():
            _lib.check(L.fs_nn_query(N, p(pred), p(perm), grid.n_total, p(grid.records), p(grid.cell_start), *grid._grid_args(), math.inf, 0,
                                     tau, p(dist2), p(index), None, None, _lib.current_stream()), "fs_nn_query")
        return call

    library(None)()
    plain = dist2.clone()
    library(order)()
    assert torch.equal(plain.view(torch.int32), dist2.view(torch.int32)), "the order of the queries changed a result"
    chunk = max(256, min(4096, (1 << 30) // N))                     # a chunk's distance matrix stays near 4 GiB
    base = cdist_nearest(pred, gt, chunk)
    diff = float((base - dist2.sqrt()).abs().max())
    m = geometry_metrics(pred, gt, (2 * vs,))

    sel = np.random.default_rng(0).choice(N, 2000, replace=False)
    ref = G.Grid(gt.cpu().numpy(), grid.lo, grid.cell, grid.dims)
    d2, _, visited = G.grid_nearest(pred.cpu().numpy()[sel], ref)
    assert np.array_equal(d2.view(np.int32), dist2.cpu().numpy()[sel].view(np.int32)), "the restatement and the kernel disagree"
    note(f"N = {N}: grid {grid.dims} cells of {grid.cell:.5f}, {visited.mean():.1f} reference points visited per query (at most {visited.max()}), "
         f"accuracy {float(m['accuracy']):.5f}, completeness {float(m['completeness']):.5f}, F-score at 2 voxels {float(m['fscore'][0]):.4f}; "
         f"max |cdist - grid| = {diff:.2e}")

    src = torch.empty(64 << 20, device=dev).normal_()
    dst = torch.empty_like(src)
    fns = {"grid_build": lambda: NearestGrid(gt), "library": library(None), "library_cell_order": library(order),
           "nearest": lambda: nearest(pred, grid), "nearest_unsorted": lambda: nearest(pred, grid, sort_queries=False),
           "geometry_metrics": lambda: geometry_metrics(pred, gt, (2 * vs,)), "copy": lambda: dst.copy_(src),
           "cdist": lambda: cdist_nearest(pred, gt, chunk)}
    calls = {"default": args.calls, "cdist": 1}
    for fn in fns.values():
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
    res = alternate(fns, calls, args.reps)
    res["copy"]["GB_per_s_read_plus_written"] = round(2.0 * src.numel() * 4 / (1e-3 * res["copy"]["median_ms"]) / 1e9, 1)
    res["cdist"]["over_nearest"] = round(res["cdist"]["median_ms"] / res["nearest"]["median_ms"], 2)
    res["cdist"]["chunk_rows"] = chunk
    return {"points_per_side": N, "grid": list(grid.dims), "cell": grid.cell, "cells": int(np.prod(grid.dims)),
            "visited_per_query_mean": round(float(visited.mean()), 2), "visited_per_query_max": int(visited.max()), "visited_sample": int(sel.size),
            "accuracy": float(m["accuracy"]), "completeness": float(m["completeness"]), "fscore_2_voxels": float(m["fscore"][0]),
            "cdist_max_abs_difference": diff, "windows": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="+", default=[200_000, 1_000_000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry_metrics_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_geometry.py needs a HIP device (no CPU fallback)")
    dev = torch.device("cuda:0")
    verts, faces, vs = mesh(dev)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "calls_per_window": args.calls,
              "mesh": {"vertices": int(verts.shape[0]), "faces": int(faces.shape[0]), "voxel_size": vs}}
    lines = []
    for N in args.sizes:
        r = result[f"{N}x{N}"] = workload(N, verts, faces, vs, args, dev)
        w = r["windows"]
        ms = lambda key: f"{w[key]['median_ms']:.2f} ms"
        lines.append(
            f"{N} sampled mesh points against {N} surface points ({r['grid'][0]} x {r['grid'][1]} x {r['grid'][2]} cells, {r['visited_per_query_mean']:.0f} "
            f"reference points visited per query, at most {r['visited_per_query_max']}): grid build {ms('grid_build')}; fs_nn_query alone {ms('library')} "
            f"with the queries in random order, {ms('library_cell_order')} in cell order; nearest() {ms('nearest')} ({ms('nearest_unsorted')} without its "
            f"sort); geometry_metrics whole {ms('geometry_metrics')}; chunked torch.cdist(...).min(1) {ms('cdist')} ({w['cdist']['over_nearest']:.0f} x "
            f"nearest()); a copy_ of 256 MiB {ms('copy')} ({w['copy']['GB_per_s_read_plus_written']:.0f} GB/s read + written).")
    result["readme"] = f"{result['device']}: " + "  ".join(lines)
    note(result["readme"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
