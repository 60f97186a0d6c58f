#!/usr/bin/env python
"""Generates tests/golden/adapter_sh{0,1,3}.npz by IMPORTING the reference (read-only at /root/reference) and running its own
GaussianAdapter(GaussianAdapterCfg(0.5, 15.0, sh_degree)).forward(fusion=False, coords=...) (gaussian_adapter.py:120-201) at
sh_degree 0, 1 and 3 -- the degrees beside make_golden.py's adapter_small.npz (sh_degree 2).  Run here only:

    python tests/golden/make_golden_sh.py

Inputs as make_golden.gen_ptf_and_adapter builds adapter_small.npz (M = 40 Gaussians, blended non-rigid extrinsics, one camera
expanded over them), seeded per degree; the raw rows have 7 + 3 d_sh channels.  Nothing here copies reference source.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import install_shim, save  # noqa: E402


def gen_adapter_sh(degree: int) -> None:
    from src.model.encoder.common.gaussian_adapter import GaussianAdapter, GaussianAdapterCfg
    h, w, M = 8, 12, 40
    torch.manual_seed(600 + degree)
    adapter = GaussianAdapter(GaussianAdapterCfg(0.5, 15.0, degree))
    d_in = adapter.d_in
    assert d_in == 7 + 3 * (degree + 1) ** 2
    E = torch.eye(4).repeat(M, 1, 1) + 0.05 * torch.randn(M, 4, 4)
    Kn = torch.tensor([[0.9, 0, 0.49], [0, 1.2, 0.51], [0, 0, 1]])
    raw = torch.randn(1, M, 1, d_in)
    dep = 1.0 + torch.rand(1, M)
    opa = torch.rand(1, M, 1, 1)
    xyz = torch.randn(1, M, 3)
    with torch.no_grad():
        # argument shapes exactly as encoder_freesplat.py:376-386 passes them
        g = adapter.forward(E.view(1, 1, M, 1, 1, 4, 4), Kn.view(1, 1, 1, 1, 1, 3, 3).expand(1, 1, M, 1, 1, 3, 3), None,
                            dep.view(1, 1, M, 1, 1), opa.view(1, 1, M, 1, 1), raw.view(1, 1, M, 1, 1, d_in), (h, w),
                            fusion=False, coords=xyz.view(1, 1, M, 1, 1, 3))
    save(f"adapter_sh{degree}.npz", extrinsics=E, intrinsics=Kn, raw=raw, depths=dep, opacities=opa, coords=xyz, h=h, w=w,
         sh_degree=degree, out_means=g.means, out_cov=g.covariances, out_harmonics=g.harmonics, out_opacities=g.opacities,
         out_scales=g.scales, out_rotations=g.rotations, sh_mask=adapter.sh_mask)


if __name__ == "__main__":
    install_shim()
    for degree in (0, 1, 3):
        gen_adapter_sh(degree)
