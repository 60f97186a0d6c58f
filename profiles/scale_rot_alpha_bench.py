"""Timings of GaussianRasterizer's (scales, rotations) form and of the alpha cotangent ("Native (scales, rotations)
covariances and the alpha gradient").

    python profiles/scale_rot_alpha_bench.py [--workload c3_968x1296_1M] [--reps 10] [--rounds 5] [--out FILE]

One view of a BASELINE workload through the drop-in GaussianRasterizer (SH degree 2, one stream):
  * scale_rot: native (scales=, rotations=; FS_RASTER_SCALE_ROT) against the eager path it replaces (build_cov3d in torch,
    then cov3D_precomp), inference forward (no_grad) and forward + backward of a colour loss;
  * alpha: forward + backward of a colour loss with and without an alpha term, and the backward alone (one forward, the
    backward replayed with retain_graph) with and without it.
Wall time per call over `reps` calls ending in a device synchronise, variants alternated within each of `rounds` rounds;
median and spread over the rounds.  Needs a HIP device (no fallback).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from freesplat_amd import synthetic  # noqa: E402
from freesplat_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer, build_cov3d  # noqa: E402
from util_raster import view_inputs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3_968x1296_1M")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    H, W, N = synthetic.WORKLOADS[a.workload]
    vi = view_inputs(synthetic.workload_scene(a.workload), synthetic.target_cameras(2), 1, H, W)
    rng = np.random.default_rng(0)
    cov = vi["cov3D"].numpy().astype(np.float64)
    size = np.sqrt(np.maximum((cov[:, 0] + cov[:, 3] + cov[:, 5]) / 3.0, 1e-12))
    scales = torch.from_numpy((size[:, None] * rng.uniform(0.3, 1.7, (N, 3))).astype(np.float32)).to(dev)
    rots = torch.from_numpy(rng.normal(size=(N, 4)).astype(np.float32)).to(dev)
    d = lambda t: t.to(dev)
    s = GaussianRasterizationSettings(H, W, vi["tanfovx"], vi["tanfovy"], d(vi["bg"]), 1.0, d(vi["viewmatrix"]),
                                      d(vi["projmatrix"]), vi["sh_degree"], d(vi["campos"]), False, False)
    rast = GaussianRasterizer(s)
    means, shs, opac = d(vi["means3D"]), d(vi["shs"]), d(vi["opacities"])[:, None]
    g_color = torch.from_numpy(rng.normal(size=(3, H, W)).astype(np.float32)).to(dev)
    g_alpha = torch.from_numpy(rng.normal(size=(H, W)).astype(np.float32)).to(dev)

    def leaves():
        return [t.detach().clone().requires_grad_(True) for t in (means, shs, opac, scales, rots)]

    def render(m, sh, op, sc, rq, native):
        if native:
            return rast(m, None, op, shs=sh, scales=sc, rotations=rq)
        return rast(m, None, op, shs=sh, cov3D_precomp=build_cov3d(sc, rq, 1.0))

    def fwd(native):
        with torch.no_grad():
            render(means, shs, opac, scales, rots, native)

    def train(native, alpha=False):
        L = leaves()
        c, _, _, al = render(*L, native)
        loss = (c * g_color).sum()
        if alpha:
            loss = loss + (al * g_alpha).sum()
        loss.backward()

    graphs = {}

    def bwd_only(alpha):
        key = alpha
        if key not in graphs:
            L = leaves()
            c, _, _, al = render(*L, True)
            loss = (c * g_color).sum() + ((al * g_alpha).sum() if alpha else 0.0)
            graphs[key] = (loss, L)
        loss, L = graphs[key]
        torch.autograd.grad(loss, L, retain_graph=True)

    variants = {
        "scale_rot_forward_native": lambda: fwd(True),
        "scale_rot_forward_eager": lambda: fwd(False),
        "scale_rot_train_native": lambda: train(True),
        "scale_rot_train_eager": lambda: train(False),
        "colour_train": lambda: train(True, False),
        "colour_alpha_train": lambda: train(True, True),
        "colour_backward": lambda: bwd_only(False),
        "colour_alpha_backward": lambda: bwd_only(True),
    }
    for fn in variants.values():       # warm-up: code objects, allocator, capacity history
        fn(); fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3 / a.reps)
    out = dict(workload=a.workload, H=H, W=W, N=N, reps=a.reps, rounds=a.rounds, device=torch.cuda.get_device_name(0),
               ms_per_call={k: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
                            for k, v in ms.items()})
    med = {k: v["median"] for k, v in out["ms_per_call"].items()}
    out["ratios"] = dict(forward_native_over_eager=round(med["scale_rot_forward_native"] / med["scale_rot_forward_eager"], 4),
                         train_native_over_eager=round(med["scale_rot_train_native"] / med["scale_rot_train_eager"], 4),
                         train_alpha_over_colour=round(med["colour_alpha_train"] / med["colour_train"], 4),
                         backward_alpha_over_colour=round(med["colour_alpha_backward"] / med["colour_backward"], 4))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
