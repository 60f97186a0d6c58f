"""Gradients with respect to camera poses and similarity transforms, through fs_sim3_tangent (libfreesplat_hip.so,
include/freesplat_amd_pose.h, csrc/gaussian_pose.hip).  The definitions are those of DESIGN.md "Pose and transform gradients":

  tangent vector xi = (u, omega, sigma), 7 numbers in that order (6: sigma = 0)
  hat(xi) = [[sigma I + [omega]x, u], [0, 0]]          Exp(xi) = matrix_exp(hat(xi)) = [[e^sigma exp([omega]x), .], [0, 1]]

Rendering a scene X from the camera E Exp(eps) equals rendering the scene moved by the inverse of that motion from E, so the
gradient of a loss with respect to a camera is a contraction of the per-Gaussian gradients the rasterizer already returns with
the generators of Sim(3): one deterministic fp64 reduction over the Gaussians (`sim3_tangent`), then a closed form
(`camera_ambient`).  The same reduction over the inputs of `transform_gaussians` and the input gradients of its backward is the
gradient with respect to the transform (`transform_ambient`; transform.py calls it when a device transform requires grad).

`observe` routes the arrays of one rendered view through an identity whose backward adds the camera's gradient; `Poses` holds
per-view corrections `delta` on top of fixed base poses.  The reduction runs on the device only; `sim3_hat`, `sim3_exp`,
`transform_ambient` and `camera_ambient` are plain torch and also run on the host.
"""
from __future__ import annotations

import torch
from torch import Tensor, nn

from . import _lib
from . import transform as X

_P = "freesplat_amd.pose: "
ARRAYS = ("means", "scales", "rotations", "covariances", "harmonics")


def _skew(w: Tensor) -> Tensor:
    """[w]x of w [..., 3] -> [..., 3, 3]."""
    x, y, z = w.unbind(-1)
    o = torch.zeros_like(x)
    return torch.stack([o, -z, y, z, o, -x, -y, x, o], -1).reshape(w.shape[:-1] + (3, 3))


def sim3_hat(xi: Tensor) -> Tensor:
    """hat(xi) [..., 4, 4] of xi [..., 7] = (u, omega, sigma), or [..., 6] with sigma = 0.  Differentiable."""
    if xi.shape[-1] not in (6, 7):
        raise ValueError(f"{_P}a tangent vector is [..., 7] = (u, omega, sigma) or [..., 6] = (u, omega), got {tuple(xi.shape)}")
    A = _skew(xi[..., 3:6])
    if xi.shape[-1] == 7:
        A = A + xi[..., 6, None, None] * torch.eye(3, dtype=xi.dtype, device=xi.device)
    top = torch.cat([A, xi[..., :3, None]], -1)
    return torch.cat([top, torch.zeros_like(top[..., :1, :])], -2)


def sim3_exp(xi: Tensor) -> Tensor:
    """Exp(xi) [..., 4, 4]: the similarity [[e^sigma exp([omega]x), V u], [0, 1]] by torch.linalg.matrix_exp.  Differentiable."""
    return torch.linalg.matrix_exp(sim3_hat(xi))


# ---- the reduction ------------------------------------------------------------------------------------------------------------

def _tangent(N: int, M: int, V: int, flags: int, ids, values, grads) -> Tensor:
    """fs_sim3_tangent on checked, contiguous float32 device tensors (None where a pair is absent) -> float64 [V, 7]."""
    L = _lib.lib()
    dev = next(g for g in grads if g is not None).device
    out = torch.empty(V, _lib.SIM3_TANGENT_DIM, dtype=torch.float64, device=dev)
    nbytes = L.fs_sim3_tangent_scratch_bytes(N, V)
    if nbytes == 0:
        raise ValueError(f"{_P}N = {N} Gaussians and {V} rows: the rows must number 1 - {_lib.SIM3_MAX_ROWS}")
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    p = _lib.ptr
    _lib.launch("fs_sim3_tangent", N, M, V, flags, p(ids), *[p(a) for a in values], *[p(g) for g in grads], p(out), p(scratch),
                nbytes)
    return out


def sim3_tangent(*, means=None, scales=None, rotations=None, covariances=None, harmonics=None, grads=None, view_ids=None,
                 rows: int = 1, quat_order: str = "wxyz", sh_layout: str = "channel_major") -> Tensor:
    """The tangent reduction: float64 [rows, 7], row v = (tau_u, tau_omega, tau_sigma) over the Gaussians with view_ids == v
    (None: all of them in row 0), for the arrays given and their gradients `grads` (a dict over "means", "scales", "rotations",
    "covariances", "harmonics"; an array without a gradient, or one that is None, adds nothing; a gradient needs its array,
    except that of the means, which then adds tau_u only).  Layouts as transform_gaussians.  Device ids are never read by
    the host, and a Gaussian with an id outside [0, rows) adds nothing.  Not differentiable; two launches, no synchronisation."""
    grads = dict(grads or {})
    unknown = set(grads) - set(ARRAYS)
    if unknown:
        raise ValueError(f"{_P}grads may hold {ARRAYS}, got {sorted(unknown)}")
    vals = dict(zip(ARRAYS, (means, scales, rotations, covariances, harmonics)))
    gs = {k: grads.get(k) for k in ARRAYS}
    for k in ARRAYS:
        if gs[k] is not None and vals[k] is None and k != "means":
            raise ValueError(f"{_P}the gradient of {k} needs {k}")
        if gs[k] is None:
            vals[k] = None
    if all(g is None for g in gs.values()):
        raise ValueError(f"{_P}no gradients given")
    shape_of = {k: (vals[k] if vals[k] is not None else gs[k]) for k in ARRAYS}
    flags, M, N, device = X._array_layout(*[None if shape_of[k] is None else shape_of[k].detach() for k in ARRAYS], quat_order, sh_layout)
    for k in ARRAYS:
        if gs[k] is not None:
            X._f32(gs[k], "the gradient of " + k)
            if vals[k] is not None and gs[k].shape != vals[k].shape:
                raise ValueError(f"{_P}the gradient of {k} must have its shape {tuple(vals[k].shape)}, got {tuple(gs[k].shape)}")
            if gs[k].device != device:
                raise ValueError(f"{_P}tensors on different devices")
    rows = int(rows)
    if not 1 <= rows <= _lib.SIM3_MAX_ROWS:
        raise ValueError(f"{_P}rows must be 1 - {_lib.SIM3_MAX_ROWS}, got {rows}")
    ids = X._ids(view_ids, N, rows, True, device)
    v = [None if vals[k] is None else vals[k].detach().contiguous() for k in ARRAYS]
    g = [None if gs[k] is None else gs[k].detach().contiguous() for k in ARRAYS]
    return _tangent(N, M, rows, flags, ids, v, g)


# ---- the closed forms ---------------------------------------------------------------------------------------------------------

def _scale_rotation(T):
    """(s [...], R [..., 3, 3]) float64 of a tuple (s, R), a library table [..., 100] or a matrix [..., 3 | 4, 4]."""
    if isinstance(T, (tuple, list)):
        if len(T) not in (2, 3):
            raise ValueError(f"{_P}a transform is (s, R), a table [V, {_lib.TRANSFORM_TABLE_FLOATS}] or a matrix [..., 3 | 4, 4]")
        s, R = X._f64(T[0]), X._f64(T[1])
        if isinstance(T[1], Tensor):
            s = s.to(T[1].device)
        return s, R
    T = X._f64(T)
    if T.shape[-1] == _lib.TRANSFORM_TABLE_FLOATS:
        return T[..., _lib.TRANSFORM_S], T[..., _lib.TRANSFORM_R:_lib.TRANSFORM_R + 9].reshape(T.shape[:-1] + (3, 3))
    if tuple(T.shape[-2:]) not in ((4, 4), (3, 4)):
        raise ValueError(f"{_P}a transform is (s, R), a table [V, {_lib.TRANSFORM_TABLE_FLOATS}] or a matrix [..., 3 | 4, 4], got "
                         f"{tuple(T.shape)}")
    A = T[..., :3, :3]
    det = torch.linalg.det(A)
    s = det.abs().pow(1.0 / 3.0) * torch.sign(det)
    return s, A / s[..., None, None]


def transform_ambient(transform, tau: Tensor) -> Tensor:
    """The gradient [..., 3, 4] with respect to the rows xf = (s R | t) of a transform T from its tangent gradient tau [..., 7]
    (sim3_tangent of the inputs of T and their gradients):

      G_A = (1 / s) R (tau_sigma / 3 I + 1/2 [tau_omega]x)        G_t = (1 / s) R tau_u

    Its inner product with every tangent direction T hat(xi) is the directional derivative tau . xi; chained through
    xf = (s R | t) by autograd it gives dL/ds = tau_sigma / s, dL/dR = s G_A, dL/dt = G_t.  `transform`: (s, R), the library's
    table [V, 100] or a matrix.  Float64, on tau's device."""
    tau = X._f64(tau)
    s, R = (x.to(tau.device) for x in _scale_rotation(transform))
    eye = torch.eye(3, dtype=torch.float64, device=tau.device)
    B = tau[..., 6, None, None] / 3.0 * eye + 0.5 * _skew(tau[..., 3:6])
    GA = (R @ B) / s[..., None, None]
    Gt = torch.einsum("...ij,...j->...i", R, tau[..., :3]) / s[..., None]
    return torch.cat([GA, Gt[..., None]], -1)


def camera_ambient(extrinsics: Tensor, tau: Tensor) -> Tensor:
    """The gradient [4, 4] with respect to a rigid camera-to-world matrix E = [R_E | t_E] from the tangent gradient tau [7] (or
    [1, 7]) of the scene it rendered, taken at the identity (sim3_tangent of the arrays and of the gradients the rasterizer
    returned for that view):

      kappa = -(tau_omega - t_E x tau_u)        G_R = 1/2 [kappa]x R_E        G_t = -tau_u        (tau_sigma is ignored)

    The last row is zero.  Float64, on tau's device."""
    if tuple(extrinsics.shape) != (4, 4):
        raise ValueError(f"{_P}extrinsics must be one [4, 4] camera-to-world matrix, got {tuple(extrinsics.shape)}")
    tau = X._f64(tau).reshape(-1)
    if tau.numel() != 7:
        raise ValueError(f"{_P}tau must be [7] or [1, 7], got {tuple(tau.shape)}")
    E = X._f64(extrinsics).to(tau.device)
    kappa = -(tau[3:6] - torch.linalg.cross(E[:3, 3], tau[:3]))
    G = torch.zeros(4, 4, dtype=torch.float64, device=tau.device)
    G[:3, :3] = 0.5 * _skew(kappa) @ E[:3, :3]
    G[:3, 3] = -tau[:3]
    return G


# ---- one rendered view --------------------------------------------------------------------------------------------------------

class _Observe(torch.autograd.Function):
    """(extrinsics, flags, M, N, means, scales, rotations, covariances, harmonics) -> the five arrays themselves."""

    @staticmethod
    def forward(ctx, extrinsics, flags, M, N, *arrays):
        ctx.save_for_backward(extrinsics, *[a for a in arrays if a is not None])
        ctx.cfg = (flags, M, N, [a is not None for a in arrays])
        ctx.set_materialize_grads(False)
        return tuple(arrays)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        flags, M, N, present = ctx.cfg
        E, *saved = ctx.saved_tensors
        g_E = None
        if ctx.needs_input_grad[0]:
            it = iter(saved)
            values = [next(it) if has else None for has in present]
            gs = [None if g is None else g.float().contiguous() for g in grads]
            values = [None if g is None else v.detach().contiguous() for v, g in zip(values, gs)]
            if any(g is not None for g in gs):
                g_E = camera_ambient(E.detach(), _tangent(N, M, 1, flags, None, values, gs)[0]).to(E.dtype)
        return (g_E, None, None, None) + tuple(grads)


def observe(extrinsics: Tensor, *, means=None, scales=None, rotations=None, covariances=None, harmonics=None,
            quat_order: str = "wxyz", sh_layout: str = "coeff_major"):
    """The arrays one view is rendered from, routed so that the view's camera receives a gradient: returns the tuple (means,
    scales, rotations, covariances, harmonics), None where None went in.

    Forward: the identity (no copy, no launch).  Backward: the arrays' gradients pass through bit for bit; when `extrinsics`
    (a device [4, 4] camera-to-world matrix, rigid) requires grad, `camera_ambient` of the tangent reduction of the arrays and
    those gradients is added to its gradient (two launches and a few small torch operations; capturable).  Render the view from
    matrices built of the SAME `extrinsics` and feed the rasterizer the returned arrays; opacities do not move with a pose and
    go to the rasterizer as they are.  `sh_layout` defaults to the rasterizer's [N, M, 3].

    One `observe` per rendered view: the camera's gradient is formed from the gradients that arrive here, so the gradients of
    several views summed into one set of leaves cannot be separated afterwards."""
    if not X._is_device(extrinsics) or tuple(extrinsics.shape) != (4, 4) or not extrinsics.dtype.is_floating_point:
        raise ValueError(f"{_P}extrinsics must be a floating [4, 4] camera-to-world matrix on a HIP device, got "
                         f"{tuple(getattr(extrinsics, 'shape', ()))} on {getattr(extrinsics, 'device', type(extrinsics))}")
    flags, M, N, device = X._array_layout(means, scales, rotations, covariances, harmonics, quat_order, sh_layout)
    if extrinsics.device != device:
        raise ValueError(f"{_P}tensors on different devices")
    return _Observe.apply(extrinsics, flags, M, N, means, scales, rotations, covariances, harmonics)


def _nearest_rotation(A: Tensor) -> Tensor:
    """The polar factor of A [..., 3, 3] (close to a rotation) by Newton's iteration X <- (X + X^-T) / 2, as the library's
    table takes it; elementwise torch only."""
    for _ in range(4):
        r0, r1, r2 = A.unbind(-2)
        C = torch.stack([torch.linalg.cross(r1, r2), torch.linalg.cross(r2, r0), torch.linalg.cross(r0, r1)], -2)   # det A^-T
        A = 0.5 * (A + C / (r0 * C[..., 0, :]).sum(-1)[..., None, None])
    return A


class Poses(nn.Module):
    """Per-view pose corrections on fixed base poses: `base` [V, 4, 4] camera-to-world matrices (a buffer, copied), `delta`
    [V, 6] (u, omega) -- or [V, 7] with scale=True -- an nn.Parameter at zero.  matrices(ids) = base @ sim3_exp(delta).

    Training: render view v from `E = poses.matrices()[v]`, route the Gaussians through `observe(E, ...)` (or
    GaussianAdam.observed(E)), and step `torch.optim.Adam([poses.delta])` beside the Gaussians' own optimizer (6 V floats do not
    warrant a kernel of their own).  fold_() moves the correction into the base; reset the optimizer's state after it."""

    def __init__(self, base: Tensor, scale: bool = False):
        super().__init__()
        if not isinstance(base, Tensor) or base.dim() != 3 or tuple(base.shape[1:]) != (4, 4) or not base.dtype.is_floating_point:
            raise ValueError(f"{_P}base must be floating [V, 4, 4] camera-to-world matrices, got {tuple(getattr(base, 'shape', ()))}")
        self.register_buffer("base", base.detach().clone())
        self.delta = nn.Parameter(torch.zeros(base.shape[0], 7 if scale else 6, dtype=base.dtype, device=base.device))

    def matrices(self, ids=None) -> Tensor:
        """[V, 4, 4], or the rows `ids` (an index, a list or a tensor of indices)."""
        base, delta = (self.base, self.delta) if ids is None else (self.base[ids], self.delta[ids])
        return base @ sim3_exp(delta)

    forward = matrices

    @torch.no_grad()
    def fold_(self) -> None:
        """base <- base Exp(delta), delta <- 0, formed in float64 with the rotation re-orthonormalised (its polar factor; with
        scale=True the scale stays in the base's linear part)."""
        T = self.base.double() @ sim3_exp(self.delta.double())
        A = T[:, :3, :3]
        s = torch.linalg.det(A).pow(1.0 / 3.0)
        T[:, :3, :3] = s[:, None, None] * _nearest_rotation(A / s[:, None, None]) if self.delta.shape[1] == 7 else _nearest_rotation(A)
        T[:, 3] = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64, device=T.device)
        self.base.copy_(T.to(self.base.dtype))
        self.delta.zero_()
