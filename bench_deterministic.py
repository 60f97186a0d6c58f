"""Cost of the deterministic mode (rasterizer.DETERMINISTIC / torch.use_deterministic_algorithms(True)): the config-3 composed
training step (bench_c3_step.bench_c3_step) and a 10-view K = 8 cost-volume training step, default and deterministic mode
alternating in one process.  Writes profiles/r9_encoder_deterministic.json (or --out) and prints one JSON line.

    python bench_deterministic.py [--rounds 3] [--steps 5] [--warmup 3] [--small]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))


def cv_train_step(dev, V=10, K=8, h=96, w=128, D=128, C=48):
    """One cost-volume forward + backward (inputs and MLP as the encoder prepares them); returns the step function."""
    import inputs
    from freesplat_amd.cost_volume import AVGFeatureVolumeManager
    torch.manual_seed(0)
    m = AVGFeatureVolumeManager(matching_height=h, matching_width=w, num_depth_bins=D, mlp_channels=[202, 32, 32, 1],
                                matching_dim_size=C).to(dev)
    kw = {k: v.to(dev) for k, v in inputs.cv_inputs(V, K, h, w, C, seed=1).items()}
    kw["cur_feats"].requires_grad_(True)
    kw["src_feats"].requires_grad_(True)
    g = torch.randn(V, D, h, w, device=dev)

    def step():
        for t in (kw["cur_feats"], kw["src_feats"], *m.parameters()):
            t.grad = None
        (m(**kw) * g).sum().backward()
    return step


def timed_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="alternations default / deterministic")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--small", action="store_true", help="config 1's size for the composed step (a quick functional run)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r9_encoder_deterministic.json"))
    a = ap.parse_args()
    from bench_c3_step import bench_c3_step
    from freesplat_amd import rasterizer as R
    dev = torch.device("cuda:0")
    c3_kw = dict(H=256, W=256, V=2, D=16) if a.small else {}
    cv = cv_train_step(dev)
    res = {"c3_step_ms": {"default": [], "deterministic": []}, "cv_10v_k8_train_ms": {"default": [], "deterministic": []}}
    for _ in range(a.rounds):
        for mode in ("default", "deterministic"):
            R.DETERMINISTIC = mode == "deterministic"
            r = bench_c3_step(dev, steps=a.steps, warmup=a.warmup, **c3_kw)
            res["c3_step_ms"][mode].append(r["ms_per_step"])
            res["cv_10v_k8_train_ms"][mode].append(timed_ms(cv, a.steps * 4, a.warmup))
    R.DETERMINISTIC = False
    out = {"metric": "deterministic-mode cost: median ms per step, default vs deterministic, alternating in one process",
           "rounds": a.rounds, "steps": a.steps, "small": a.small, "device": torch.cuda.get_device_name(dev)}
    for k, v in res.items():
        d, t = statistics.median(v["default"]), statistics.median(v["deterministic"])
        out[k] = {"default_median": d, "deterministic_median": t, "ratio": t / d, "default": v["default"],
                  "deterministic": v["deterministic"]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("c3_step_ms", "cv_10v_k8_train_ms")}, separators=(",", ":")))


if __name__ == "__main__":
    main()
