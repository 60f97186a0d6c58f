#!/usr/bin/env python
"""Generates tests/golden/mv_depth_small.npz by IMPORTING the reference (read-only, make_golden.py's REF) and running its
MVDepthLoss and ScaleInvariantLoss (src/loss/losses.py) in float64 on the CPU, on two small decidable cases of
tests/mv_depth_cases.py.  Run where the reference is, only:

    python tests/golden/make_mv_depth_golden.py

Nothing below copies reference source: it stubs the reference's missing third-party imports the way make_golden.py does
(install_shim), imports its module and calls it.  The file holds the inputs, the two loss values and autograd's gradients with
respect to the predicted depth; tests/test_mv_depth_loss_host.py compares tests/mv_depth_ref.py with them.

The reference back-projects pixel x + 0.5 with K's own cx and samples its half-pixel coordinate u at the pixel round(u - 0.5)
(grid_sample, nearest, align_corners=False): both are this project's convention with cx - 0.5, cy - 0.5, for the current view
and for the source.  The cases keep the integer-pixel intrinsics; the reference receives them with 0.5 added.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import make_golden  # noqa: E402
import mv_depth_cases as MC  # noqa: E402

CASES = {"a": (9, 11, 3, 2, 2), "b": (16, 20, 1, 1, 1)}        # name -> (H, W, K, views, seed) of MC.golden_case


def import_losses():
    make_golden.install_shim()
    for name, path in (("src.loss", "src/loss"), ("src.loss.utils", "src/loss/utils")):     # (bare packages: no __init__ runs)
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(make_golden.REF, path)]
        sys.modules[name] = m
    from src.loss import losses
    return losses


def K44(k, views, lead=()):
    """(fx, fy, cx, cy) of integer-pixel coordinates -> the reference's 4 x 4 K in half-pixel coordinates."""
    K = torch.eye(4, dtype=torch.float64)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = k[0], k[1], k[2] + 0.5, k[3] + 0.5
    return K.expand(views, *lead, 4, 4).contiguous()


def main():
    losses = import_losses()
    out = {}
    for name, (H, W, K, views, seed) in CASES.items():
        c = MC.golden_case(H, W, K, views, seed)
        MC.assert_decidable(c)
        cams = c["cams"]
        pred = c["depth"].double().requires_grad_(True)
        gt, src = c["gt"].double(), c["src"].double()
        mv = losses.MVDepthLoss(H, W).double()
        loss = mv(pred[:, None], gt[:, None], src[:, :, None], torch.linalg.inv(K44(cams["intr"], views)), K44(cams["src_intr"], views, (K,)),
                  cams["cam_to_world"], cams["src_world_to_cam"])
        g_mv, = torch.autograd.grad(loss, pred)
        assert bool(torch.isfinite(loss)) and float(loss.detach()) > 0
        mask = torch.isfinite(gt) & (gt > 0)
        si = losses.ScaleInvariantLoss().double()(torch.log(gt[mask]), torch.log(pred[mask]))
        g_si, = torch.autograd.grad(si, pred)
        assert bool(torch.isfinite(si)) and float(si.detach()) > 0
        arrs = dict(depth=c["depth"], gt=c["gt"], src=c["src"], intr=cams["intr"], cam_to_world=cams["cam_to_world"],
                    src_intr=cams["src_intr"], src_world_to_cam=cams["src_world_to_cam"], pairs=c["pairs"], mv_loss=loss.detach(),
                    mv_grad=g_mv, si_loss=si.detach(), si_grad=g_si, holed=torch.tensor(c["holed"]))
        out.update({f"{name}_{k}": v.detach().numpy() for k, v in arrs.items()})
        print(name, (H, W, K, views), "mv", float(loss.detach()), "si", float(si.detach()), "holed", c["holed"])
    path = os.path.join(HERE, "mv_depth_small.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
