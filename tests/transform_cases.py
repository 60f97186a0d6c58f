"""Shared cases of the similarity-transform tests (tests/test_transform_host.py, tests/test_transform_hip.py, the smoke line).

Sizes sit where the kernels change path: a thread owns four Gaussians in the geometry arrays and one (M = 16) or four in the
harmonics, a workgroup 256 threads -- 1 (a lone, partial run), 63 / 64 / 65 (around a wavefront of runs of one), 257 (a
second workgroup's first thread at M = 16, a partial last run everywhere else), 1000 (a whole workgroup of runs of four, minus
a few)."""
from __future__ import annotations

import math

import torch

import transform_ref as TR

NS = (1, 63, 64, 65, 257, 1000)
MS = (1, 4, 9, 16)
VS = (1, 3)
EPS = 2.0 ** -24          # unit roundoff of fp32


def transforms(V: int, seed: int = 0) -> torch.Tensor:
    """xf [V,3,4] float32: rows (s R | t) with s in 0.4 - 2.5, a random rotation (the first one with w < 0 before the sign
    choice: an angle beyond pi about a random axis), t of a few units."""
    g = torch.Generator().manual_seed(100 + seed)
    rows = []
    for v in range(V):
        R = TR.random_rotation(g)
        s = math.exp(float(torch.empty(1, dtype=torch.float64).uniform_(math.log(0.4), math.log(2.5), generator=g)))
        t = 3.0 * torch.randn(3, dtype=torch.float64, generator=g)
        rows.append(torch.cat([s * R, t[:, None]], 1))
    return torch.stack(rows).float()


def ids_for(N: int, V: int, seed: int = 0):
    """None for V == 1 on even seeds; else [N] int64 over [-1, V]: both out-of-range values occur when N >= 8."""
    if V == 1 and seed % 2 == 0:
        return None
    g = torch.Generator().manual_seed(200 + seed)
    ids = torch.randint(0, V, (N,), generator=g)
    if N >= 8:
        ids[1], ids[N - 2], ids[N // 2] = -1, V, -1
    return ids


def arrays(N: int, M: int, seed: int = 0, cov_full: bool = False, sh_layout: str = "coeff_major") -> dict:
    """float32 means [N,3], scales [N,3], rotations [N,4] (norms 0.5 - 2), cov [N,6] or [N,3,3] (3 x 3: NOT symmetric, the
    kernel must not assume it), shs [N,M,3] or [N,3,M]."""
    g = torch.Generator().manual_seed(300 + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    q = r(N, 4)
    q = q / q.norm(dim=1, keepdim=True) * (0.5 + 1.5 * torch.rand(N, 1, generator=g))
    shs = r(N, M, 3) * (0.5 ** torch.arange(M).float().sqrt().floor())[None, :, None]
    return dict(means=4.0 * r(N, 3), scales=torch.exp(r(N, 3)), rotations=q, cov=r(N, 3, 3) if cov_full else r(N, 6),
                shs=shs if sh_layout == "coeff_major" else shs.transpose(1, 2).contiguous())


def gamma(n: int) -> float:
    """Higham's gamma_n = n u / (1 - n u) for fp32."""
    return n * EPS / (1.0 - n * EPS)


def band_bound(c_l: torch.Tensor, l: int) -> torch.Tensor:
    """2 (2l + 3) 2^-24 |c_l|_2 per (Gaussian, channel): 2l + 1 FMAs and the rounding of D, margin 2.  c_l [N, 2l+1, 3]
    float64 (coefficient-major) -> [N, 1, 3]."""
    return 2.0 * (2 * l + 3) * EPS * c_l.norm(dim=1, keepdim=True)


# ---- the rendering invariance -------------------------------------------------------------------------------------------------

FX_N, FY_N = 1170.0 / 1296.0, 1170.0 / 968.0        # normalised focal lengths (freesplat_amd.synthetic), principal point centred


def camera_matrices(c2w: torch.Tensor, near: float, far: float):
    """float64 (viewmatrix, projmatrix, campos, tanfovx, tanfovy) in the rasterizer's row-vector convention, built as the decoder
    frames a view (symmetric frustum, x / y -> (-1, 1), w = z) but in float64 throughout."""
    tx, ty = 0.5 / FX_N, 0.5 / FY_N
    P = torch.zeros(4, 4, dtype=torch.float64)
    P[0, 0], P[1, 1], P[3, 2] = 1.0 / tx, 1.0 / ty, 1.0
    P[2, 2], P[2, 3] = far / (far - near), -(far * near) / (far - near)
    view = torch.linalg.inv(c2w.double()).T.contiguous()
    return view, (view @ P.T).contiguous(), c2w[:3, 3].double().contiguous(), tx, ty


def invariance_scene(N: int = 100, depth: float = 1000.0, seed: int = 5, sh_degree: int = 3) -> dict:
    """A tiny (scales, rotations) scene in front of one camera, float64.  Depths are 0.6 - 1.4 of `depth`, sizes are a few pixels
    at 24 x 32 and larger.

    Why depths of about 1000 units: oracle/raster_dense_torch.render_dense divides by (w + 1e-7).  That guard is not
    scale-invariant; at depth z a similarity of scale s moves a projected centre by 1e-7 (1 - 1 / s) / z of its NDC coordinate.
    At z >= 600 that is below 1e-10 of the image, two orders under the 1e-9 bound of the invariance test, so the test judges the
    transform and not the guard.  (Every depth is far above the near cull at 0.2 max(1, s).)"""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, dtype=torch.float64, generator=g)
    r = lambda *s: torch.randn(*s, dtype=torch.float64, generator=g)
    c2w = torch.eye(4, dtype=torch.float64)
    c2w[:3, :3] = TR.random_rotation(g)
    c2w[:3, 3] = depth * 0.3 * r(3)
    z = depth * (0.6 + 0.8 * u(N))
    cam = torch.stack([(2 * u(N) - 1) * 0.5 / FX_N * z, (2 * u(N) - 1) * 0.5 / FY_N * z, z], 1)
    means = cam @ c2w[:3, :3].T + c2w[:3, 3]
    scales = z[:, None] / 32.0 / FX_N * (1.0 + 3.0 * u(N, 3))            # 1 - 4 pixels of a 32-pixel-wide image
    q = r(N, 4)
    M = (sh_degree + 1) ** 2
    shs = 0.4 * r(N, M, 3)
    shs[:, 0] = 1.5 * r(N, 3)
    return dict(means=means, scales=scales, rotations=q / q.norm(dim=1, keepdim=True) * (0.5 + u(N, 1)),
                opacities=0.05 + 0.85 * u(N), shs=shs, c2w=c2w, near=0.01 * depth, far=10.0 * depth, sh_degree=sh_degree)


def render_scene(N: int = 600, seed: int = 11, sh_degree: int = 3) -> dict:
    """The 64 x 80 scene of the GaussianAdam.transform_ render test: invariance_scene at depths of 2.4 - 5.6 units (the near
    cull at 0.2 max(1, s) is far away), rounded to float32, opacities below 0.9."""
    sc = invariance_scene(N, depth=4.0, seed=seed, sh_degree=sh_degree)
    sc["scales"] = sc["scales"] * 0.5                                     # 64 x 80: 1 - 5 pixels
    return {k: (v.float() if isinstance(v, torch.Tensor) else v) for k, v in sc.items()}


def oracle_render(sc: dict, means, scales, rotations, shs, c2w, H=64, W=80):
    """The C oracle's fp32 forward of (scales, rotations) Gaussians -> (color [3,H,W], depth [H,W]) numpy."""
    import numpy as np
    from freesplat_amd.rasterizer import build_cov3d
    from oracle import raster_oracle as ro
    view, proj, campos, tx, ty = camera_matrices(c2w, sc["near"], sc["far"])
    n = lambda t: t.detach().float().cpu().numpy()
    st = ro.forward(H, W, tx, ty, np.array([0.2, 0.3, 0.1], np.float32), n(view), n(proj), sc["sh_degree"], n(campos), n(means),
                    n(build_cov3d(scales.float(), rotations.float(), 1.0)), n(sc["opacities"]), shs=n(shs))
    return st["color"], st["depth"]
