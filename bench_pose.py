#!/usr/bin/env python
"""Pose and transform gradient benchmark (standalone; not the headline metric).  One process, everything warmed first.

1.0 M Gaussians at SH degree 3: means, scales, rotations, harmonics [N,16,3] and their gradients, 2 x 58 floats per Gaussian.

  library    fs_sim3_tangent alone (device events around back-to-back calls on preallocated buffers), one row and 64 rows with
             the ids in runs; it only reads: 2 x 58 floats per Gaussian, 464 MB at 1.0 M, which is its bound in bytes (the fp64
             arithmetic, about 300 multiply-adds per Gaussian, is small beside a pass over those bytes)
  copy       dst.copy_(src) of 2 x 58 floats per Gaussian (reads them and writes as many), and src.sum() of the same floats (a
             read-only pass): the rates a pass over these bytes reaches in this session
  transform  transform_gaussians forward + backward of all four arrays, with a transform that does not require grad and with one
             that does (the difference is the reduction, its scratch and the closed form)
  render     one 968 x 1296 view of the synthetic 1.0 M scene, forward + backward of the colour image, from the optimizer's
             leaves and through GaussianAdam.observed with extrinsics that require grad
  eager      the reduction as a user writes it in torch (cross products, one einsum with the generators, .sum(0)), in float32 and
             on float64 copies of the arrays.  A yardstick, not code under test

The windows alternate inside one session (--calls per window; ten times as many for the library call, the copy and the sum, a
third for eager and render); the median window and the spread (min, max) of the per-call times are reported, and
the library call's bytes over its time as a share of the copy's rate (bytes read + written over its time).

Prints one JSON object and writes it to --out.    python bench_pose.py [--n 1000000 --reps 7 --out profiles/pose_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch


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


def camera_matrices(c2w, near, far, fx_n, fy_n):
    """(viewmatrix, projmatrix, campos, tanfovx, tanfovy) in the rasterizer's row-vector convention, float32 on c2w's device."""
    tx, ty = 0.5 / fx_n, 0.5 / fy_n
    P = torch.zeros(4, 4, dtype=torch.float64)
    P[0, 0], P[1, 1], P[3, 2] = 1.0 / tx, 1.0 / ty, 1.0
    P[2, 2], P[2, 3] = far / (far - near), -(far * near) / (far - near)
    view = torch.linalg.inv(c2w.detach().double().cpu()).T.contiguous()
    f = lambda t: t.float().to(c2w.device)
    return f(view), f(view @ P.T), f(c2w.detach()[:3, 3].double().cpu()), tx, ty


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose.py needs a HIP device (no CPU fallback)")
    from freesplat_amd import _lib, synthetic
    from freesplat_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    from freesplat_amd.refine import GaussianAdam
    from freesplat_amd.transform import transform_gaussians
    dev = torch.device("cuda:0")
    N, M = args.n, 16
    g = torch.Generator(dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    order = ("means", "scales", "rotations", "cov", "shs")
    a = dict(means=r(N, 3), scales=torch.exp(r(N, 3)), rotations=r(N, 4), cov=None, shs=r(N, M, 3))
    gr = dict(means=r(N, 3), scales=r(N, 3), rotations=r(N, 4), cov=None, shs=r(N, M, 3))
    floats = sum(v.numel() for v in a.values() if v is not None)
    result = {"device": torch.cuda.get_device_name(0), "N": N, "sh_degree": 3, "reps": args.reps, "calls_per_window": args.calls,
              "floats_read_per_gaussian": 2 * floats // N, "bytes_read": 2 * 4 * floats}
    L, p = _lib.lib(), _lib.ptr

    # ---- the library call alone
    def library(V):
        ids = None if V == 1 else (torch.arange(N, device=dev) * V // N).to(torch.int64)
        nbytes = L.fs_sim3_tangent_scratch_bytes(N, V)
        out = torch.empty(V, 7, dtype=torch.float64, device=dev)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)

        def call():
            _lib.check(L.fs_sim3_tangent(N, M, V, 0, p(ids), *[p(a[k]) for k in order], *[p(gr[k]) for k in order], p(out), p(scratch),
                                         nbytes, _lib.current_stream()), "fs_sim3_tangent")
        call.keep = (ids, out, scratch)
        return call

    src = torch.empty(2 * floats, device=dev).normal_()
    dst = torch.empty_like(src)

    # ---- transform_gaussians, with and without the transform's gradient
    q = r(4)
    q = q / q.norm()
    w, x, y, z = q.tolist()
    R = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], device=dev)
    T = torch.eye(4, device=dev)
    T[:3, :3], T[:3, 3] = 1.7 * R, torch.tensor([0.5, -1.0, 2.0], device=dev)
    leaves = {k: v.clone().requires_grad_(True) for k, v in a.items() if v is not None}

    def transform(with_grad):
        Tl = T.clone().requires_grad_(with_grad)

        def step():
            out = [o for o in transform_gaussians(None, Tl, means=leaves["means"], scales=leaves["scales"], rotations=leaves["rotations"],
                                                  harmonics=leaves["shs"], sh_layout="coeff_major") if o is not None]
            torch.autograd.backward(out, [gr[k] for k in order if gr[k] is not None])
            Tl.grad = None
            for v in leaves.values():
                v.grad = None
        return step

    # ---- the eager form of the reduction
    buf = (C.c_double * (3 * 83))()
    _lib.check(L.fs_sim3_sh_generators(buf), "fs_sim3_sh_generators")
    flat = torch.tensor(list(buf), dtype=torch.float64).reshape(3, 83)
    G = torch.zeros(3, 16, 16, dtype=torch.float64)
    for l, off in ((1, 0), (2, 9), (3, 34)):
        n = 2 * l + 1
        G[:, l * l:l * l + n, l * l:l * l + n] = flat[:, off:off + n * n].reshape(3, n, n)

    def eager(dtype):
        Gd = G.to(dev, dtype)

        def step():
            m, s, qq, sh = (a[k].to(dtype) for k in ("means", "scales", "rotations", "shs"))
            gm, gs, gq, gsh = (gr[k].to(dtype) for k in ("means", "scales", "rotations", "shs"))
            qw, qv, gw, gv = qq[:, :1], qq[:, 1:], gq[:, :1], gq[:, 1:]
            om = (torch.linalg.cross(m, gm) + 0.5 * (qw * gv - gw * qv + torch.linalg.cross(qv, gv))).sum(0)
            om = om + (gsh[:, None] * torch.einsum("kij,njc->nkic", Gd, sh)).sum((0, 2, 3))
            sg = (m * gm).sum() + (s * gs).sum()
            return torch.cat([gm.sum(0), om, sg[None]])
        return step

    fns = {"library_1_row": library(1), "library_64_rows": library(64), "copy": lambda: dst.copy_(src), "read_only_sum": lambda: src.sum(),
           "transform_forward_backward": transform(False), "transform_forward_backward_with_transform_grad": transform(True),
           "eager_float32": eager(torch.float32), "eager_float64": eager(torch.float64)}
    calls = {"default": args.calls, **{k: 10 * args.calls for k in ("library_1_row", "library_64_rows", "copy", "read_only_sum")},
             "eager_float32": max(2, args.calls // 3), "eager_float64": max(2, args.calls // 3)}

    # ---- one 968 x 1296 render, with and without observe
    H, W, _ = synthetic.WORKLOADS["c3_968x1296_1M"]
    sc = synthetic.make_scene(N, sh_degree=3)
    opt = GaussianAdam.from_gaussians(types.SimpleNamespace(**{k: sc[k].to(dev) for k in ("means", "covariances", "harmonics", "opacities")}))
    cam = synthetic.target_cameras(1)
    E0 = cam["extrinsics"][0].to(dev)
    view, proj, campos, tx, ty = camera_matrices(E0, 0.5, 15.0, synthetic.FX_N, synthetic.FY_N)
    st = GaussianRasterizationSettings(H, W, tx, ty, torch.zeros(3, device=dev), 1.0, view, proj, 3, campos, False, False)
    rast = GaussianRasterizer(st)

    def render(observed):
        E = E0.clone().requires_grad_(observed)

        def step():
            means, scales, rotations, opacities, shs = opt.observed(E) if observed else opt.leaves()
            out = rast(means3D=means, means2D=torch.zeros_like(means), opacities=opacities, shs=shs, scales=scales, rotations=rotations)
            out[0].sum().backward()
            E.grad = None
            opt.zero_grad()
        return step

    fns["render_forward_backward"], fns["render_forward_backward_observed"] = render(False), render(True)
    calls["render_forward_backward"] = calls["render_forward_backward_observed"] = max(2, args.calls // 3)

    for k, fn in fns.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        note(f"warmed {k}")
    note(f"{2 * floats // N} floats read per Gaussian, {2 * 4 * floats / 1e6:.0f} MB")
    res = alternate(fns, calls, args.reps)
    nbytes = 2.0 * 4 * floats
    copy_rate = 2.0 * nbytes / (1e-3 * res["copy"]["median_ms"])               # the copy reads nbytes and writes nbytes
    res["copy"]["GB_per_s_read_plus_written"] = round(copy_rate / 1e9, 1)
    res["read_only_sum"]["GB_per_s"] = round(nbytes / (1e-3 * res["read_only_sum"]["median_ms"]) / 1e9, 1)
    for k in ("library_1_row", "library_64_rows"):
        rate = nbytes / (1e-3 * res[k]["median_ms"])
        res[k]["GB_per_s"] = round(rate / 1e9, 1)
        res[k]["share_of_copy_rate"] = round(rate / copy_rate, 3)
    result["windows"] = res
    ms = lambda k: f"{res[k]['median_ms']:.2f} ms" if k in res else "not measured"
    result["readme"] = (
        f"{N / 1e6:.1f} M Gaussians at SH degree 3 ({result['device']}): fs_sim3_tangent alone {ms('library_1_row')} "
        f"({res['library_1_row']['GB_per_s']:.0f} GB/s over the {nbytes / 1e6:.0f} MB it reads = "
        f"{100 * res['library_1_row']['share_of_copy_rate']:.0f} % of the rate of a copy_ of those bytes, {ms('copy')}, "
        f"{res['copy']['GB_per_s_read_plus_written']:.0f} GB/s read + written; a read-only sum of them {ms('read_only_sum')}), "
        f"{ms('library_64_rows')} with 64 rows; transform_gaussians forward + backward {ms('transform_forward_backward')}, with the "
        f"transform's gradient {ms('transform_forward_backward_with_transform_grad')}; one 968 x 1296 render forward + backward "
        f"{ms('render_forward_backward')}, through observe {ms('render_forward_backward_observed')}; the reduction in eager torch "
        f"{ms('eager_float32')} in float32, {ms('eager_float64')} in float64.")
    note(result["readme"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
