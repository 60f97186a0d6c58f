"""Float64 restatement of the Sim(3) tangent reduction (include/freesplat_amd_pose.h, csrc/gaussian_pose.hip) in plain torch,
independent of the library and of freesplat_amd.pose.

The infinitesimal similarity x -> x + sigma x + omega x x + u moves every array linearly (the means also by the constant u):

  means  sigma mu + omega x mu + u      scales  sigma s      rotations  1/2 (0, omega) (x) q
  cov    2 sigma S + [omega]x S - S [omega]x                 shs        sum_k omega_k G_{l,k} c_l per band and channel

Each motion is written out as the contract states it, applied to the unit vectors of one Gaussian's floats to get the matrix
A_e of tangent direction e (7 of them), and the reduction is tau_e = sum_i g_i^T A_e x_i.  The SH generators come from autograd
of transform_ref.rotate_sh(., matrix_exp([omega]x)) at omega = 0 -- the least-squares D_l of that file, nothing shared with
the kernel's constants.

`tangent` also returns the bound of the GPU tests: for each output, 4 n 2^-53 S with n the number of scalar summands behind it
(the nonzero entries of A_e times the Gaussians that count) and S the sum of their absolute values, sum_i |g_i|^T |A_e| |x_i|."""
from __future__ import annotations

import torch

import transform_ref as TR

F64 = torch.float64
ARRAYS = ("means", "scales", "rotations", "cov", "shs")
U53 = 2.0 ** -53


def skew(w: torch.Tensor) -> torch.Tensor:
    x, y, z = w.unbind(-1)
    o = torch.zeros_like(x)
    return torch.stack([o, -z, y, z, o, -x, -y, x, o], -1).reshape(w.shape[:-1] + (3, 3))


def hat(xi: torch.Tensor) -> torch.Tensor:
    """[[sigma I + [omega]x, u], [0, 0]] of xi [7] = (u, omega, sigma)."""
    H = torch.zeros(4, 4, dtype=F64)
    H[:3, :3] = xi[6] * torch.eye(3, dtype=F64) + skew(xi[3:6])
    H[:3, 3] = xi[:3]
    return H


_GEN = None


def generators() -> torch.Tensor:
    """[3, 16, 16] float64: block-diagonal G_{l,k} over the 16 coefficients (band 0: zero), k = x, y, z."""
    global _GEN
    if _GEN is None:
        basis = torch.eye(16, dtype=F64)[:, :, None].expand(16, 16, 3).contiguous()          # Gaussian n holds e_n in every channel

        def D(w):
            return TR.rotate_sh(basis, torch.linalg.matrix_exp(skew(w))[None])[:, :, 0].T      # out[n, i] = D[i, n]

        J = torch.autograd.functional.jacobian(D, torch.zeros(3, dtype=F64))                  # [16, 16, 3]
        _GEN = J.permute(2, 0, 1).contiguous()
    return _GEN


def generator_table() -> torch.Tensor:
    """[3, 83]: the D_1, D_2, D_3 block layout of a table row, per axis."""
    G = generators()
    return torch.stack([torch.cat([G[k, l * l:(l + 1) ** 2, l * l:(l + 1) ** 2].reshape(-1) for l in (1, 2, 3)]) for k in range(3)])


def motion(kind: str, x: torch.Tensor, xi: torch.Tensor, quat_order="wxyz", sh_layout="coeff_major") -> torch.Tensor:
    """The linear part of the motion of one array under xi [7]; x [N, ...] float64 in the array's own layout."""
    u, w, sg = xi[:3], xi[3:6], xi[6]
    if kind == "means":
        return sg * x + torch.linalg.cross(w.expand_as(x), x)
    if kind == "scales":
        return sg * x
    if kind == "rotations":
        q = x if quat_order == "wxyz" else x[:, [3, 0, 1, 2]]
        d = 0.5 * TR.quat_mul(torch.cat([torch.zeros(1, dtype=F64), w]).expand_as(q), q)
        return d if quat_order == "wxyz" else d[:, [1, 2, 3, 0]]
    if kind == "cov":
        S = x if x.dim() == 3 else TR.cov6_to_mat(x)
        d = 2.0 * sg * S + skew(w) @ S - S @ skew(w)
        return d if x.dim() == 3 else TR.mat_to_cov6(d)
    if kind == "shs":
        c = x if sh_layout == "coeff_major" else x.transpose(1, 2)                             # [N, M, 3]
        M = c.shape[1]
        A = torch.einsum("k,kij->ij", w, generators())[:M, :M]
        d = torch.einsum("ij,njc->nic", A, c)
        return d if sh_layout == "coeff_major" else d.transpose(1, 2)
    raise ValueError(kind)


def operators(kind: str, shape, quat_order="wxyz", sh_layout="coeff_major") -> torch.Tensor:
    """A [7, W, W]: A[e] maps the W floats of one Gaussian (shape `shape`) to their motion under tangent direction e."""
    W = 1
    for s in shape:
        W *= s
    basis = torch.eye(W, dtype=F64).reshape((W,) + tuple(shape))
    A = torch.stack([motion(kind, basis, torch.eye(7, dtype=F64)[e], quat_order, sh_layout).reshape(W, W).T for e in range(7)])
    A[A.abs() < 1e-14] = 0.0
    return A


def tangent(V: int, ids, values: dict, grads: dict, quat_order="wxyz", sh_layout="coeff_major"):
    """(tau [V, 7], bound [V, 7]) float64.  values / grads: dicts over ARRAYS (missing or None: nothing); ids [N] or None (all
    in row 0).  The gradient of the means may come without the means (tau_u only)."""
    tau, S, n = _reduce(V, ids, values, grads, quat_order, sh_layout)
    return tau, 4.0 * n * U53 * S


def pushed(V: int, ids, values: dict, bounds: dict, quat_order="wxyz", sh_layout="coeff_major") -> torch.Tensor:
    """Elementwise bounds |dg| <= bounds on the gradients, pushed through the (linear) reduction: [V, 7], sum_i b_i^T |A_e| |x_i|."""
    return _reduce(V, ids, values, bounds, quat_order, sh_layout)[1]


def _reduce(V, ids, values, grads, quat_order, sh_layout):
    tau, S, n = (torch.zeros(V, 7, dtype=F64) for _ in range(3))
    for k in ARRAYS:
        g = grads.get(k)
        if g is None:
            continue
        g = g.detach().to(F64)
        N = g.shape[0]
        ids_ = torch.zeros(N, dtype=torch.int64) if ids is None else torch.as_tensor(ids).to(torch.int64)
        gf = g.reshape(N, -1)
        for v in range(V):
            on = ids_ == v
            if k == "means":
                tau[v, :3] += gf[on].sum(0)
                S[v, :3] += gf[on].abs().sum(0)
                n[v, :3] += int(on.sum())
            x = values.get(k)
            if x is None:
                assert k == "means", k
                continue
            x = x.detach().to(F64)
            A = operators(k, x.shape[1:], quat_order, sh_layout)
            xf = x.reshape(N, -1)
            tau[v] += torch.einsum("ni,eij,nj->e", gf[on], A, xf[on])
            S[v] += torch.einsum("ni,eij,nj->e", gf[on].abs(), A.abs(), xf[on].abs())
            n[v] += int(on.sum()) * (A != 0).sum((1, 2)).to(F64)
    return tau, S, n
