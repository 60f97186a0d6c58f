#!/usr/bin/env python
"""Generates tests/golden/depth_metrics.npz by IMPORTING the reference (read-only at /root/reference) and running its own
depth_render_metrics (src/model/model_wrapper.py:90-110) and compute_psnr (src/evaluation/metrics.py:11-19) on seeded
inputs.  Run here only:

    python tests/golden/make_golden_metrics.py

Importing those two modules needs stubs beyond make_golden.install_shim's: the third-party packages model_wrapper and
metrics import at module level (pytorch_lightning, wandb, lpips, skimage.metrics, moviepy, mmcv) and the reference's own
modules model_wrapper pulls in for training and visualisation.  None of them is called by the two functions.

Cases (arrays <case>__gt / __pred [b, v, h, w], outputs <case>__abs_diff / __abs_rel / __delta_25 / __delta_10):
  mixed     b = 2, v = 3: every edge case of the NaN rules on a few pixels of each view (gt == 0.5, gt NaN, pred NaN,
            pred = 0, negative pred, ratios on both sides of 1.25 and 1.1)
  single    b = 1, v = 2: plain positive depths
  empty     b = 1, v = 2: the second view has no valid pixel (NaN propagates into the means)
  inf_pred  b = 1, v = 1: pred = +inf on one valid pixel (abs terms infinite)
PSNR: psnr__gt / psnr__pred [4, 3, 24, 32] with values outside [0, 1] (view 3 identical: inf), psnr__out [4].
"""
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, install_shim  # noqa: E402


class _Stub:
    def __init__(self, *a, **k):
        pass

    def __call__(self, *a, **k):
        return self


def _stub_module(name):
    m = types.ModuleType(name)
    m.__path__ = []

    def getattr_(attr):
        if attr.startswith("__"):
            raise AttributeError(attr)
        return type(attr, (_Stub,), {})
    m.__getattr__ = getattr_
    sys.modules[name] = m
    return m


def install_metric_stubs():
    for name in ("moviepy", "moviepy.editor", "wandb", "pytorch_lightning", "pytorch_lightning.loggers",
                 "pytorch_lightning.loggers.wandb", "pytorch_lightning.utilities", "mmcv", "lpips", "skimage",
                 "skimage.metrics",
                 "src.dataset.data_module", "src.global_cfg", "src.loss", "src.misc", "src.misc.benchmarker",
                 "src.misc.image_io", "src.misc.LocalLogger", "src.misc.step_tracker", "src.visualization",
                 "src.visualization.annotation", "src.visualization.camera_trajectory",
                 "src.visualization.camera_trajectory.interpolation", "src.visualization.camera_trajectory.wobble",
                 "src.visualization.color_map", "src.visualization.layout", "src.visualization.validation_in_3d",
                 "src.model.decoder.decoder", "src.model.encoder.encoder_freesplat",
                 "src.model.encoder.visualization.encoder_visualizer"):
        _stub_module(name)
    sys.modules["src.model.encoder"].Encoder = type("Encoder", (_Stub,), {})
    sys.modules["src.misc.LocalLogger"].LOG_PATH = "."


def depth_cases():
    g = torch.Generator().manual_seed(20261015)
    u = lambda *s: torch.rand(*s, generator=g)
    cases = {}
    b, v, h, w = 2, 3, 16, 20
    gt = 0.2 + 4.8 * u(b, v, h, w)
    pred = gt * (1 + 0.3 * (u(b, v, h, w) - 0.5))
    # edge pixels of every view, at fixed rows
    gt[..., 0, 0] = 0.5                      # invalid (the mask is gt > 0.5)
    gt[..., 0, 1] = float("nan")             # invalid
    pred[..., 0, 2] = float("nan")           # valid, dropped from the abs terms, "not within delta"
    pred[..., 0, 3] = 0.0                    # infinite ratio
    pred[..., 0, 4] = -1.0                   # negative: passes the delta test, as in the reference
    gt[..., 1, :4] = 2.0
    pred[..., 1, 0] = 2.0 * 1.249           # inside 1.25, outside 1.1
    pred[..., 1, 1] = 2.0 / 1.26            # outside both
    pred[..., 1, 2] = 2.0 * 1.099           # inside both
    pred[..., 1, 3] = 2.0                   # exact
    gt[..., 2, :3] = torch.tensor([0.5000001, 0.4999999, 0.0])
    cases["mixed"] = (gt, pred)
    gt = 0.6 + 3 * u(1, 2, 12, 14)
    cases["single"] = (gt, gt * (1 + 0.2 * (u(1, 2, 12, 14) - 0.5)))
    gt = 0.6 + 3 * u(1, 2, 12, 14)
    gt[0, 1] = 0.3
    cases["empty"] = (gt, gt * 1.05)
    gt = 0.6 + 3 * u(1, 1, 12, 14)
    pred = gt * 1.02
    pred[0, 0, 3, 3] = float("inf")
    cases["inf_pred"] = (gt, pred)
    return cases


def main():
    install_shim()
    install_metric_stubs()
    import importlib
    mw = importlib.import_module("src.model.model_wrapper")
    em = importlib.import_module("src.evaluation.metrics")
    out = {}
    for name, (gt, pred) in depth_cases().items():
        batch = {"target": {"depth": gt.unsqueeze(2).clone()}}
        res = mw.depth_render_metrics(types.SimpleNamespace(depth=pred.clone()), batch)
        out[f"{name}__gt"], out[f"{name}__pred"] = gt.numpy(), pred.numpy()
        for k, r in zip(("abs_diff", "abs_rel", "delta_25", "delta_10"), res):
            out[f"{name}__{k}"] = r.numpy()
        print(name, [float(r) for r in res])
    gen = torch.Generator().manual_seed(7)
    gt = torch.rand(4, 3, 24, 32, generator=gen) * 1.6 - 0.3
    pred = (gt + 0.1 * torch.randn(4, 3, 24, 32, generator=gen)).clone()
    pred[3] = gt[3]
    out["psnr__gt"], out["psnr__pred"] = gt.numpy(), pred.numpy()
    out["psnr__out"] = em.compute_psnr(gt, pred).numpy()
    print("psnr", out["psnr__out"])
    np.savez_compressed(os.path.join(OUT, "depth_metrics.npz"), **out)


if __name__ == "__main__":
    main()
