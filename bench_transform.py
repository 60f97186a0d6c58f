#!/usr/bin/env python
"""Similarity-transform benchmark (standalone; not the headline metric).  One process, everything warmed first.

1.0 M Gaussians at SH degree 3, one transform for all.  Two sets of arrays: "scene" = means, scales, rotations, harmonics
[N,16,3] (58 floats per Gaussian in and out; opacities do not change and are not touched) and "scene+cov" = the same plus world
covariances [N,3,3].

  fused    freesplat_amd.transform.transform_gaussians under no_grad (out of place), the same + backward of all arrays, and the
           in-place form GaussianAdam.transform_ uses (the library call with out == in) -- ms per call including the Python
           wrapper and the table launch; beside them the library call alone (device events around back-to-back calls on
           preallocated buffers, table prepared once)
  eager    what a user writes today in fp32 torch on the same device: s * means @ R^T + t, s * scales, the quaternion product,
           R @ cov @ R^T, one einsum per SH band with D_l from sh_rotation_matrices -- forward under no_grad, and forward +
           backward under autograd.  A yardstick, not code under test
  copy     dst.copy_(src) of the same number of floats: the rate a pass over these bytes can reach

Fused, eager and copy windows alternate inside one session; the median window and the spread (min, max) of the per-call times
are reported, and each library call's bytes (read + written) over its time as a share of the copy's rate.

Prints one JSON object and writes it to --out.    python bench_transform.py [--n 1000000 --reps 7 --out profiles/transform_bench.json]
"""
import argparse
import json
import os
import sys

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
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(window_ms(fn, calls))
    stat = lambda v: {"median_ms": round(sorted(v)[len(v) // 2], 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    return {k: stat(v) for k, v in times.items()}


def quat_mul(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transform_bench.json"))
    args = ap.parse_args()
    from freesplat_amd import _lib
    from freesplat_amd.transform import prepare_table, sh_rotation_matrices, transform_gaussians
    dev = torch.device("cuda:0")
    N, M = args.n, 16
    g = torch.Generator(dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    q = r(4)
    q = q / q.norm()
    w, x, y, z = q.tolist()
    R = torch.tensor([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], device=dev)
    s, t = 1.7, torch.tensor([0.5, -1.0, 2.0], device=dev)
    T = torch.eye(4, device=dev)
    T[:3, :3], T[:3, 3] = s * R, t
    D = [d.float() for d in sh_rotation_matrices(R, 3)]
    base = dict(means=r(N, 3), scales=torch.exp(r(N, 3)), rotations=r(N, 4), shs=r(N, M, 3), cov=r(N, 3, 3))
    table = prepare_table(T[None, :3].contiguous())
    result = {"device": torch.cuda.get_device_name(0), "N": N, "sh_degree": 3, "reps": args.reps, "calls_per_window": args.calls, "sets": {}}
    for name, keys in (("scene", ("means", "scales", "rotations", "shs")), ("scene+cov", ("means", "scales", "rotations", "cov", "shs"))):
        a = {k: base[k] for k in keys}
        floats = sum(v.numel() for v in a.values())
        kw = lambda d: dict(means=d["means"], scales=d["scales"], rotations=d["rotations"], covariances=d.get("cov"), harmonics=d["shs"],
                            sh_layout="coeff_major")
        leaves = {k: v.clone().requires_grad_(True) for k, v in a.items()}
        ones = {k: torch.ones_like(v) for k, v in a.items()}

        def fused_fwd():
            with torch.no_grad():
                return transform_gaussians(None, T, **kw(a))

        def fused_train():
            out = [o for o in transform_gaussians(None, T, **kw(leaves)) if o is not None]
            torch.autograd.backward(out, [torch.ones_like(o) for o in out])
            for v in leaves.values():
                v.grad = None

        order = ("means", "scales", "rotations", "cov", "shs")
        ins = [a.get(k) for k in order]
        outs = [None if v is None else torch.empty_like(v) for v in ins]
        work = [None if v is None else v.clone() for v in ins]
        p, L, flags = _lib.ptr, _lib.lib(), _lib.TRANSFORM_COV_FULL

        def lib_call(which, i, o):
            _lib.check(getattr(L, "fs_gaussians_transform_" + which)(N, M, 1, flags, p(table), None, *[p(v) for v in i], *[p(v) for v in o],
                                                                    _lib.current_stream()), which)

        def fused_inplace():
            prepare_table(T[None, :3].contiguous())
            lib_call("forward", work, work)

        def eager(d):
            out = [s * d["means"] @ R.T + t, s * d["scales"], quat_mul(q, d["rotations"])]
            if "cov" in d:
                out.append((s * s) * (R @ d["cov"] @ R.T))
            sh = d["shs"]
            out.append(torch.cat([sh[:, :1]] + [torch.einsum("ij,njc->nic", D[l], sh[:, l * l:(l + 1) ** 2]) for l in (1, 2, 3)], 1))
            return out

        def eager_fwd():
            with torch.no_grad():
                return eager(a)

        def eager_train():
            out = eager(leaves)
            torch.autograd.backward(out, [torch.ones_like(o) for o in out])
            for v in leaves.values():
                v.grad = None

        src = torch.empty(floats, device=dev).normal_()
        dst = torch.empty_like(src)
        fns = {"fused_forward": fused_fwd, "fused_forward_backward": fused_train, "fused_in_place": fused_inplace,
               "library_forward": lambda: lib_call("forward", ins, outs), "library_forward_in_place": lambda: lib_call("forward", work, work),
               "library_backward": lambda: lib_call("backward", ins, outs), "eager_forward": eager_fwd,
               "eager_forward_backward": eager_train, "copy": lambda: dst.copy_(src)}
        for fn in fns.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        note(f"{name}: {floats / N:.0f} floats per Gaussian, {2 * 4 * floats / 1e6:.0f} MB read + written")
        res = alternate(fns, args.calls, args.reps)
        nbytes = 2.0 * 4 * floats
        rate = lambda k: nbytes / (1e-3 * res[k]["median_ms"])
        for k in ("library_forward", "library_forward_in_place", "library_backward", "copy"):
            res[k]["GB_per_s"] = round(rate(k) / 1e9, 1)
            res[k]["share_of_copy_rate"] = round(rate(k) / rate("copy"), 3)
        res["floats_per_gaussian"] = floats // N
        res["bytes_read_and_written"] = int(nbytes)
        result["sets"][name] = res
        del src, dst
    sc = result["sets"]["scene"]
    result["readme"] = (
        f"{N / 1e6:.1f} M Gaussians at SH degree 3 ({result['device']}): transform_gaussians {sc['fused_forward']['median_ms']:.2f} ms forward, "
        f"{sc['fused_forward_backward']['median_ms']:.2f} ms forward + backward, {sc['fused_in_place']['median_ms']:.2f} ms in place "
        f"(library call alone {sc['library_forward']['median_ms']:.2f} ms, {sc['library_forward']['GB_per_s']:.0f} GB/s = "
        f"{100 * sc['library_forward']['share_of_copy_rate']:.0f} % of a copy_ of the same bytes at {sc['copy']['median_ms']:.2f} ms); "
        f"eager fp32 torch {sc['eager_forward']['median_ms']:.2f} ms forward, {sc['eager_forward_backward']['median_ms']:.2f} ms forward + backward.")
    note(result["readme"])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
