"""Float64 restatement of the similarity transform of Gaussians (include/freesplat_amd_transform.h, csrc/gaussian_transform.hip)
in plain torch, independent of the library and of freesplat_amd.transform.

D_l comes from the DEFINING identity b_l(R d) = D_l b_l(d): the bands of the rasterizer's basis (the formulas of
oracle/raster_dense_torch._sh_color, term by term) are evaluated at 64 fixed random directions and at their rotated images,
and D_l is the least-squares solution of D_l B = B' -- no quadrature, no Wigner recursion, nothing shared with the kernel's
construction.  Everything else is the contract written out: means, scales, the Hamilton product, R S R^T.  All functions are
differentiable by autograd in the Gaussians."""
from __future__ import annotations

import math

import torch

from oracle.raster_dense_torch import C0, C1, C2, C3

F64 = torch.float64
TABLE_FLOATS = 100
OFF = dict(s=0, R=1, t=10, q=13, D1=17, D2=26, D3=51)
TRIU = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def band(l: int, d: torch.Tensor) -> torch.Tensor:
    """b_l at directions d [..., 3] -> [..., 2l+1]: the factors that multiply shs[:, l*l + i] in _sh_color."""
    x, y, z = d.unbind(-1)
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    if l == 0:
        return torch.full_like(x, C0)[..., None]
    if l == 1:
        return torch.stack([-C1 * y, C1 * z, -C1 * x], -1)
    if l == 2:
        return torch.stack([C2[0] * xy, C2[1] * yz, C2[2] * (2 * zz - xx - yy), C2[3] * xz, C2[4] * (xx - yy)], -1)
    return torch.stack([C3[0] * y * (3 * xx - yy), C3[1] * xy * z, C3[2] * y * (4 * zz - xx - yy),
                        C3[3] * z * (2 * zz - 3 * xx - 3 * yy), C3[4] * x * (4 * zz - xx - yy), C3[5] * z * (xx - yy),
                        C3[6] * x * (xx - 3 * yy)], -1)


def _directions(n=64, seed=1234):
    d = torch.randn(n, 3, dtype=F64, generator=torch.Generator().manual_seed(seed))
    return d / d.norm(dim=-1, keepdim=True)


_DIRS = _directions()


def sh_matrix(l: int, R: torch.Tensor) -> torch.Tensor:
    """D_l(R) [2l+1, 2l+1] float64 from the defining identity, by least squares over 64 directions."""
    R = R.to(F64)
    B = band(l, _DIRS)                      # [K, n]: rows b_l(d_k)^T
    Bp = band(l, _DIRS @ R.T)               # rows b_l(R d_k)^T = b_l(d_k)^T D^T
    return torch.linalg.lstsq(B, Bp).solution.T


def random_rotation(gen) -> torch.Tensor:
    q = torch.randn(4, dtype=F64, generator=gen)
    return quat_to_matrix(q / q.norm())


def quat_to_matrix(q: torch.Tensor) -> torch.Tensor:
    """(w, x, y, z) of any norm -> the rotation of the normalised quaternion [..., 3, 3] (the rasterizer's build_cov3d form)."""
    q = q / q.norm(dim=-1, keepdim=True)
    r, x, y, z = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], -1).reshape(q.shape[:-1] + (3, 3))


def matrix_to_quat(R: torch.Tensor) -> torch.Tensor:
    """The unit quaternion (w, x, y, z) of a rotation with w >= 0, through the eigenvector of the largest eigenvalue of the
    4 x 4 matrix of Bar-Itzhack's method (not the four-candidate branch the kernel uses)."""
    R = R.to(F64)
    m = lambda i, j: R[i, j]
    K = torch.stack([
        torch.stack([m(0, 0) - m(1, 1) - m(2, 2), m(1, 0) + m(0, 1), m(2, 0) + m(0, 2), m(2, 1) - m(1, 2)]),
        torch.stack([m(1, 0) + m(0, 1), m(1, 1) - m(0, 0) - m(2, 2), m(2, 1) + m(1, 2), m(0, 2) - m(2, 0)]),
        torch.stack([m(2, 0) + m(0, 2), m(2, 1) + m(1, 2), m(2, 2) - m(0, 0) - m(1, 1), m(1, 0) - m(0, 1)]),
        torch.stack([m(2, 1) - m(1, 2), m(0, 2) - m(2, 0), m(1, 0) - m(0, 1), m(0, 0) + m(1, 1) + m(2, 2)])]) / 3.0
    w, V = torch.linalg.eigh(K)
    x, y, z, r = V[:, -1]
    q = torch.stack([r, x, y, z])
    return -q if float(q[0]) < 0 else q


def quat_mul(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Hamilton product a (x) b of (w, x, y, z) quaternions [..., 4]."""
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], -1)


def split_xf(xf: torch.Tensor):
    """xf [V,3,4] (the fp32 rows (s R | t) the library gets) -> float64 (s [V], R [V,3,3], t [V,3]) as the header defines them:
    s = cbrt(det), R the rotation nearest to the linear part over s -- the fp32 entries are a rotation only to 2^-24, and D_l and
    q_R are defined for rotations."""
    A = xf[:, :, :3].to(F64)
    det = torch.linalg.det(A)
    s = det.abs().pow(1.0 / 3.0) * torch.sign(det)
    U, _, Vh = torch.linalg.svd(A / s[:, None, None])         # the nearest rotation: the polar factor U V^T (det > 0 for a similarity)
    return s, U @ Vh, xf[:, :, 3].to(F64)


def table(xf: torch.Tensor) -> torch.Tensor:
    """The [V, 100] float64 table of xf [V,3,4]."""
    s, R, t = split_xf(xf)
    rows = []
    for v in range(xf.shape[0]):
        rows.append(torch.cat([s[v:v + 1], R[v].reshape(-1), t[v], matrix_to_quat(R[v])]
                              + [sh_matrix(l, R[v]).reshape(-1) for l in (1, 2, 3)]))
    return torch.stack(rows)


def _resolve(ids, N, V):
    ids = torch.zeros(N, dtype=torch.int64) if ids is None else torch.as_tensor(ids).to(torch.int64)
    return ids, (ids >= 0) & (ids < V)


def rotate_sh(sh, R, ids=None, layout="coeff_major", transpose=False):
    """sh [N,M,3] ("coeff_major") or [N,3,M]; R [V,3,3] float64; ids [N] or None.  Out-of-range ids pass through."""
    sh = sh.to(F64)
    c = sh if layout == "coeff_major" else sh.transpose(1, 2)            # [N, M, 3]
    N, M = c.shape[0], c.shape[1]
    ids, on = _resolve(ids, N, R.shape[0])
    out = [c[:, :1]]
    for l in range(1, int(round(math.sqrt(M)))):
        D = torch.stack([sh_matrix(l, R[v]) for v in range(R.shape[0])])   # [V, n, n]
        if transpose:
            D = D.transpose(1, 2)
        cl = c[:, l * l:(l + 1) * (l + 1)]
        rot = torch.einsum("nij,njc->nic", D[ids.clamp(0, R.shape[0] - 1)], cl)
        out.append(torch.where(on[:, None, None], rot, cl))
    out = torch.cat(out, 1)
    return out if layout == "coeff_major" else out.transpose(1, 2)


def cov6_to_mat(c6):
    rows = [[c6[:, 0], c6[:, 1], c6[:, 2]], [c6[:, 1], c6[:, 3], c6[:, 4]], [c6[:, 2], c6[:, 4], c6[:, 5]]]
    return torch.stack([torch.stack(r, -1) for r in rows], -2)


def mat_to_cov6(S):
    return torch.stack([S[:, i, j] for i, j in TRIU], -1)


def transform(xf, ids=None, means=None, scales=None, rotations=None, cov=None, shs=None, quat_order="wxyz", sh_layout="coeff_major"):
    """The forward of the contract in float64; returns the five outputs (None where None went in).  Differentiable."""
    s, R, t = split_xf(xf)
    V = xf.shape[0]
    N = next(a.shape[0] for a in (means, scales, rotations, cov, shs) if a is not None)
    ids, on = _resolve(ids, N, V)
    k = ids.clamp(0, V - 1)
    out = [None] * 5
    if means is not None:
        m = means.to(F64)
        out[0] = torch.where(on[:, None], s[k, None] * torch.einsum("nij,nj->ni", R[k], m) + t[k], m)
    if scales is not None:
        sc = scales.to(F64)
        out[1] = torch.where(on[:, None], s[k, None] * sc, sc)
    if rotations is not None:
        q = rotations.to(F64)
        qw = q if quat_order == "wxyz" else q[:, [3, 0, 1, 2]]
        qr = torch.stack([matrix_to_quat(R[v]) for v in range(V)])
        r = quat_mul(qr[k], qw)
        r = r if quat_order == "wxyz" else r[:, [1, 2, 3, 0]]
        out[2] = torch.where(on[:, None], r, q)
    if cov is not None:
        c = cov.to(F64)
        if c.dim() == 2:
            r = mat_to_cov6((s[k] ** 2)[:, None, None] * (R[k] @ cov6_to_mat(c) @ R[k].transpose(1, 2)))
            out[3] = torch.where(on[:, None], r, c)
        else:
            r = (s[k] ** 2)[:, None, None] * (R[k] @ c @ R[k].transpose(1, 2))
            out[3] = torch.where(on[:, None, None], r, c)
    if shs is not None:
        out[4] = rotate_sh(shs, R, ids, sh_layout)
    return out


def transform_cameras(c2w, s, R, t):
    """c2w' = [R R_c | s R c + t] in float64."""
    c2w = c2w.to(F64)
    out = c2w.clone()
    out[..., :3, :3] = R @ c2w[..., :3, :3]
    out[..., :3, 3] = s * (c2w[..., :3, 3] @ R.T) + t
    return out
