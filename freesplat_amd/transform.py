"""Similarity transforms of Gaussian scenes on the device, through fs_transform_prepare, fs_sh_rotate and
fs_gaussians_transform_forward / _backward (libfreesplat_hip.so, include/freesplat_amd_transform.h,
csrc/gaussian_transform.hip).  The definitions are those of DESIGN.md "Similarity transforms":

  transform T = (s, R, t), s > 0, R a proper rotation: x -> s R x + t
  means' = s R means + t        scales' = s scales        q' = q_R (x) q  (Hamilton product, q_R the unit quaternion of R, w >= 0)
  cov' = s^2 R cov R^T          opacities unchanged       SH band l of every colour channel: c'_l = D_l(R) c_l
  D_l(R): b_l(R d) = D_l(R) b_l(d) for every unit d, b_l the band of the basis the rasterizer evaluates (D_0 = 1)

Rendering the transformed scene from `transform_cameras(extrinsics, T)` gives the same colour image and s times the depth.

The SH blocks are this project's own: they are defined by the rasterizer's basis (its order, constants and signs), not by the
Wigner matrices of another library's basis order.

A transform is a 4 x 4 matrix [s R | t; 0 0 0 1] (or its first three rows) or a tuple (s, R, t); [V, 4, 4] / (s [V], R [V,3,3], t [V,3]) with `view_ids`
gives every Gaussian its own transform.  A HOST transform (CPU tensor, array, numbers) is checked in float64 -- R^T R = I,
det > 0, s > 0 -- and raises ValueError; a DEVICE tensor is taken as given, without synchronisation (capturable in a graph).

Gradients reach the Gaussians and, in `transform_gaussians`, a DEVICE transform that requires grad (a matrix, or the tensors of
(s, R, t); with `view_ids` up to 64 rows): the backward then also runs the tangent reduction of pose.py over the inputs and
their gradients and hands autograd the ambient gradient of the rows (s R | t) (DESIGN.md "Pose and transform gradients").  The
gradient is that of a similarity: it is exact along T Exp(xi) and has no component that would shear the matrix.  A transform
that does not require grad costs what it did, and a host transform never receives a gradient.  Device tensors only: there is
no CPU / eager path.
"""
from __future__ import annotations

import dataclasses
import math

import torch
from torch import Tensor

from . import _lib

_P = "freesplat_amd.transform: "
_ORTHO_TOL = 1e-5          # |R^T R - I| of a host transform: fp32 matrices pass, a shear of 1e-4 does not
SH_LAYOUTS = ("channel_major", "coeff_major")        # [..., 3, M] (the adapter's harmonics) / [..., M, 3] (the rasterizer's shs)
QUAT_ORDERS = ("wxyz", "xyzw")

_C1 = 0.4886025119029199
_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
       1.445305721320277, -0.5900435899266435)


def _band(l: int, d: Tensor) -> Tensor:
    """b_l of the rasterizer's basis at unit directions d [..., 3] -> [..., 2l + 1]."""
    x, y, z = d.unbind(-1)
    if l == 0:
        return torch.full_like(x, 0.28209479177387814)[..., None]
    if l == 1:
        return torch.stack([-_C1 * y, _C1 * z, -_C1 * x], -1)
    xx, yy, zz = x * x, y * y, z * z
    if l == 2:
        return torch.stack([_C2[0] * x * y, _C2[1] * y * z, _C2[2] * (2 * zz - xx - yy), _C2[3] * x * z, _C2[4] * (xx - yy)], -1)
    if l == 3:
        return torch.stack([_C3[0] * y * (3 * xx - yy), _C3[1] * x * y * z, _C3[2] * y * (4 * zz - xx - yy),
                            _C3[3] * z * (2 * zz - 3 * xx - 3 * yy), _C3[4] * x * (4 * zz - xx - yy), _C3[5] * z * (xx - yy),
                            _C3[6] * x * (xx - 3 * yy)], -1)
    raise ValueError(f"{_P}SH bands 0 - 3 only, got {l}")


def _lebedev26(device):
    a, b = math.sqrt(0.5), math.sqrt(1.0 / 3.0)
    pts = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    pts += [(0, p * a, q * a) for p in (1, -1) for q in (1, -1)] + [(p * a, 0, q * a) for p in (1, -1) for q in (1, -1)]
    pts += [(p * a, q * a, 0) for p in (1, -1) for q in (1, -1)]
    pts += [(p * b, q * b, r * b) for p in (1, -1) for q in (1, -1) for r in (1, -1)]
    w = [1 / 21] * 6 + [4 / 105] * 12 + [9 / 280] * 8
    return torch.tensor(pts, dtype=torch.float64, device=device), torch.tensor(w, dtype=torch.float64, device=device)


def sh_rotation_matrices(R, degree: int = 3) -> list:
    """[D_0, ..., D_degree] for the rotation(s) R [..., 3, 3]: float64 tensors [..., 2l+1, 2l+1] on R's device with
    b_l(R d) = D_l b_l(d).  The same construction as the library's table (the degree-7 Lebedev rule integrates
    b_l(R d) b_l(d)^T exactly), in plain torch: for inspection and for composing with other code, not a hot path."""
    if not 0 <= int(degree) <= 3:
        raise ValueError(f"{_P}degree must be 0 - 3, got {degree}")
    R = _f64(R)
    if R.shape[-2:] != (3, 3):
        raise ValueError(f"{_P}R must be [..., 3, 3], got {tuple(R.shape)}")
    d, w = _lebedev26(R.device)
    rd = torch.einsum("...ij,kj->...ki", R, d)
    return [4 * math.pi * torch.einsum("k,...ki,kj->...ij", w, _band(l, rd), _band(l, d)) for l in range(int(degree) + 1)]


# ---- transforms ---------------------------------------------------------------------------------------------------------------

def _f64(x) -> Tensor:
    """float64 without a detour through float32 (torch.as_tensor(1.7) is a float32 tensor)."""
    return x.double() if isinstance(x, Tensor) else torch.as_tensor(x, dtype=torch.float64)


def _split_host(T) -> tuple:
    """A host transform -> float64 (s [V], R [V,3,3], t [V,3], batched?) after the checks."""
    if isinstance(T, (tuple, list)) and len(T) == 3:
        s, R, t = (_f64(x) for x in T)
        batched = R.dim() == 3
        if R.shape[-2:] != (3, 3) or R.dim() not in (2, 3):
            raise ValueError(f"{_P}R must be [3, 3] or [V, 3, 3], got {tuple(R.shape)}")
        R = R.reshape(-1, 3, 3)
        V = R.shape[0]
        if s.numel() not in (1, V) or t.numel() not in (3, 3 * V):
            raise ValueError(f"{_P}(s, R, t) must be a number or [V], [V, 3, 3], [3] or [V, 3]; got {tuple(s.shape)}, {tuple(R.shape)}, {tuple(t.shape)}")
        s, t = s.reshape(-1).expand(V), t.reshape(-1, 3).expand(V, 3)
    else:
        M = _f64(T)
        if tuple(M.shape[-2:]) not in ((4, 4), (3, 4)) or M.dim() not in (2, 3):
            raise ValueError(f"{_P}a transform is a 4 x 4 matrix (or its first three rows), [V, 4, 4] or a tuple (s, R, t); got "
                             f"shape {tuple(M.shape)}")
        batched = M.dim() == 3
        M = M.reshape(-1, M.shape[-2], 4)
        if M.shape[1] == 4 and not torch.equal(M[:, 3], torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64).expand(M.shape[0], 4)):
            raise ValueError(f"{_P}the last row of a transform must be (0, 0, 0, 1), got {M[:, 3].tolist()}")
        A, t = M[:, :3, :3], M[:, :3, 3]
        det = torch.linalg.det(A)
        if not bool((det > 0).all()) or not bool(torch.isfinite(M).all()):
            raise ValueError(f"{_P}not a similarity: det of the linear part is {det.tolist()} (a reflection, a zero scale or a "
                             "non-finite entry)")
        s = det.pow(1.0 / 3.0)
        R = A / s[:, None, None]
    if not bool(torch.isfinite(s).all() and torch.isfinite(R).all() and torch.isfinite(t).all()):
        raise ValueError(f"{_P}a transform must be finite")
    if not bool((s > 0).all()):
        raise ValueError(f"{_P}the scale of a similarity must be > 0, got {s.tolist()}")
    err = float((R.transpose(1, 2) @ R - torch.eye(3, dtype=torch.float64)).abs().max())
    if err > _ORTHO_TOL:
        raise ValueError(f"{_P}not a similarity: R^T R differs from the identity by {err:.3g} (sheared or non-uniformly scaled)")
    if not bool((torch.linalg.det(R) > 0).all()):
        raise ValueError(f"{_P}not a similarity: det R < 0 (a reflection)")
    return s, R, t, batched


def _is_device(x) -> bool:
    return isinstance(x, Tensor) and x.device.type == "cuda"


def _xf(T, device) -> tuple:
    """transform -> (xf [V, 3, 4] float32 on `device`, rows (s R | t), detached; batched?)."""
    xf, batched, _ = _xf_live(T, device)
    return xf, batched


def _xf_live(T, device) -> tuple:
    """As _xf, and third the same rows attached to the autograd graph of a device transform that requires grad (else None)."""
    parts = T if isinstance(T, (tuple, list)) and len(T) == 3 else (T,)
    if any(_is_device(x) for x in parts):
        if len(parts) == 3:
            s, R, t = (torch.as_tensor(x, dtype=torch.float32, device=device) for x in parts)
            if R.shape[-2:] != (3, 3) or R.dim() not in (2, 3):
                raise ValueError(f"{_P}R must be [3, 3] or [V, 3, 3], got {tuple(R.shape)}")
            batched = R.dim() == 3
            R = R.reshape(-1, 3, 3)
            V = R.shape[0]
            if s.numel() not in (1, V) or t.numel() not in (3, 3 * V):
                raise ValueError(f"{_P}(s, R, t) must be a number or [V], [V, 3, 3], [3] or [V, 3]; got {tuple(s.shape)}, {tuple(R.shape)}, {tuple(t.shape)}")
            xf = torch.cat([s.reshape(-1, 1, 1).expand(V, 1, 1) * R, t.reshape(-1, 3, 1).expand(V, 3, 1)], 2)
        else:
            M = parts[0]
            if tuple(M.shape[-2:]) not in ((4, 4), (3, 4)) or M.dim() not in (2, 3):
                raise ValueError(f"{_P}a transform is a 4 x 4 matrix (or its first three rows), [V, 4, 4] or a tuple (s, R, t); "
                                 f"got shape {tuple(M.shape)}")
            batched = M.dim() == 3
            xf = M.reshape(-1, M.shape[-2], 4)[:, :3, :]
        if xf.device != device:
            raise ValueError(f"{_P}tensors on different devices")
        live = xf.float().contiguous() if torch.is_grad_enabled() and xf.requires_grad else None
        return xf.detach().float().contiguous(), batched, live
    s, R, t, batched = _split_host(T)
    xf = torch.cat([s[:, None, None] * R, t[:, :, None]], 2)
    return xf.float().to(device), batched, None


def prepare_table(xf: Tensor) -> Tensor:
    """xf [V, 3, 4] float32 on the device, rows (s R | t) -> the library's table [V, 100] (fs_transform_prepare)."""
    V = xf.shape[0]
    table = torch.empty(V, _lib.TRANSFORM_TABLE_FLOATS, dtype=torch.float32, device=xf.device)
    _lib.launch("fs_transform_prepare", V, _lib.ptr(xf), _lib.ptr(table))
    return table


def _ids(view_ids, N: int, V: int, batched: bool, device):
    """None (one transform for all) or [N] int64 on the device.  Device ids are trusted (an id outside [0, V) passes its
    Gaussian through); host ids are range-checked."""
    if view_ids is None:
        if V != 1:
            raise ValueError(f"{_P}{V} transforms need view_ids")
        return None
    if _is_device(view_ids):
        ids = view_ids
        if ids.device != device:
            raise ValueError(f"{_P}tensors on different devices")
    else:
        ids = torch.as_tensor(view_ids)
    if ids.dtype.is_floating_point or ids.dtype.is_complex or ids.dtype == torch.bool:
        raise ValueError(f"{_P}view_ids must be integers, got {ids.dtype}")
    if ids.numel() != N:
        raise ValueError(f"{_P}view_ids must have one entry per Gaussian ({N}), got {tuple(ids.shape)}")
    ids = ids.detach().reshape(N).to(torch.int64)
    if not _is_device(view_ids):
        if bool(((ids < 0) | (ids >= V)).any()):
            raise ValueError(f"{_P}view_ids must lie in [0, {V})")
        ids = ids.to(device)
    return ids.contiguous()


def _f32(t, what: str) -> Tensor:
    if not _is_device(t):
        raise ValueError(f"{_P}{what} must be a tensor on a HIP device (got {getattr(t, 'device', type(t))}); there is no CPU path")
    if t.dtype != torch.float32:
        raise ValueError(f"{_P}{what} must be float32, got {t.dtype}")
    if t.numel() == 0:
        raise ValueError(f"{_P}{what} is empty: {tuple(t.shape)}")
    return t


def _sh_dims(sh: Tensor, layout: str):
    if layout not in SH_LAYOUTS:
        raise ValueError(f"{_P}layout must be one of {SH_LAYOUTS}, got {layout!r}")
    if sh.dim() < 2:
        raise ValueError(f"{_P}harmonics must be [..., 3, M] or [..., M, 3], got {tuple(sh.shape)}")
    three, M = (sh.shape[-2], sh.shape[-1]) if layout == "channel_major" else (sh.shape[-1], sh.shape[-2])
    if three != 3 or M not in (1, 4, 9, 16):
        want = "[..., 3, M]" if layout == "channel_major" else "[..., M, 3]"
        raise ValueError(f"{_P}harmonics must be {want} with M in (1, 4, 9, 16) for layout {layout!r}, got {tuple(sh.shape)}")
    return int(M), sh.numel() // (3 * int(M))


class _Transform(torch.autograd.Function):
    """(xf, table, ids, flags, M, N, means, scales, rotations, cov, shs) -> the five transformed arrays (None where None went
    in).  xf: None, or the rows (s R | t) the table was made of when they require grad; the inputs are then kept (by reference)
    for the tangent reduction of the backward."""

    @staticmethod
    def forward(ctx, xf, table, ids, flags, M, N, *arrays):
        ins = [None if a is None else a.contiguous() for a in arrays]
        outs = [None if a is None else torch.empty_like(a) for a in ins]
        p = _lib.ptr
        _lib.launch("fs_gaussians_transform_forward", N, M, table.shape[0], flags, p(table), p(ids), *[p(a) for a in ins],
                    *[p(a) for a in outs])
        ctx.save_for_backward(table, *([ids] if ids is not None else []), *([a for a in ins if a is not None] if xf is not None else []))
        ctx.cfg = (flags, M, N, ids is not None, [a is not None for a in ins], xf is not None)
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        flags, M, N, has_ids, present, has_xf = ctx.cfg
        table = ctx.saved_tensors[0]
        ids = ctx.saved_tensors[1] if has_ids else None
        need_xf = has_xf and ctx.needs_input_grad[0]              # the transform's gradient needs every array's input gradient
        needs = ctx.needs_input_grad[6:]
        gs = [None if (g is None or not (need or need_xf)) else g.float().contiguous() for g, need in zip(grads, needs)]
        if all(g is None for g in gs):
            return (None,) * 11
        outs = [None if g is None else torch.empty_like(g) for g in gs]
        p = _lib.ptr
        _lib.launch("fs_gaussians_transform_backward", N, M, table.shape[0], flags, p(table), p(ids), *[p(g) for g in gs],
                    *[p(o) for o in outs])
        g_xf = None
        if need_xf:
            from . import pose
            it = iter(ctx.saved_tensors[2 if has_ids else 1:])
            ins = [next(it) if has else None for has in present]
            ins = [None if o is None else a for a, o in zip(ins, outs)]
            tau = pose._tangent(N, M, table.shape[0], flags, ids, ins, outs)
            g_xf = pose.transform_ambient(table, tau).float()
        return (g_xf,) + (None,) * 5 + tuple(o if need else None for o, need in zip(outs, needs))


class _RotateSH(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sh, table, ids, flags, M, N):
        sh = sh.contiguous()
        out = torch.empty_like(sh)
        p = _lib.ptr
        _lib.launch("fs_sh_rotate", N, M, table.shape[0], flags, p(sh), p(table), p(ids), p(out))
        ctx.save_for_backward(table, *([ids] if ids is not None else []))
        ctx.cfg = (flags, M, N, ids is not None)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        flags, M, N, has_ids = ctx.cfg
        table = ctx.saved_tensors[0]
        ids = ctx.saved_tensors[1] if has_ids else None
        g = g.float().contiguous()
        out = torch.empty_like(g)
        p = _lib.ptr
        _lib.launch("fs_sh_rotate", N, M, table.shape[0], flags ^ _lib.TRANSFORM_SH_TRANSPOSE, p(g), p(table), p(ids), p(out))
        return out, None, None, None, None, None


def rotate_sh(sh: Tensor, rotations, view_ids=None, layout: str = "channel_major", transpose: bool = False) -> Tensor:
    """Rotate spherical harmonics with the frame: band l of every colour channel becomes D_l(R) c_l.  sh [..., 3, M]
    (layout "channel_major", the adapter's harmonics) or [..., M, 3] ("coeff_major", the rasterizer's shs), M in (1, 4, 9, 16);
    rotations [3, 3], or [V, 3, 3] with view_ids (one per Gaussian: integers in [0, V); on the device they are never read by
    the host, and a Gaussian with an id outside the range is passed through).  transpose=True applies D_l^T, the inverse
    rotation.  Differentiable with respect to sh."""
    sh = _f32(sh, "harmonics")
    M, N = _sh_dims(sh, layout)
    if _is_device(rotations):
        if rotations.shape[-2:] != (3, 3) or rotations.dim() not in (2, 3):
            raise ValueError(f"{_P}rotations must be [3, 3] or [V, 3, 3], got {tuple(rotations.shape)}")
        if rotations.device != sh.device:
            raise ValueError(f"{_P}tensors on different devices")
        batched = rotations.dim() == 3
        R = rotations.detach().float().reshape(-1, 3, 3)
        xf = torch.cat([R, torch.zeros(R.shape[0], 3, 1, dtype=torch.float32, device=sh.device)], 2).contiguous()
    else:
        xf, batched = _xf((1.0, rotations, torch.zeros(3, dtype=torch.float64)), sh.device)
    ids = _ids(view_ids, N, xf.shape[0], batched, sh.device)
    flags = (_lib.TRANSFORM_SH_CHANNEL_MAJOR if layout == "channel_major" else 0) | (_lib.TRANSFORM_SH_TRANSPOSE if transpose else 0)
    return _RotateSH.apply(sh, prepare_table(xf), ids, flags, M, N)


def transform_gaussians(gaussians=None, transform=None, *, means=None, scales=None, rotations=None, covariances=None,
                        harmonics=None, view_ids=None, quat_order: str = "wxyz", sh_layout: str = "channel_major"):
    """Apply the similarity `transform` to Gaussians.

    Dataclass form, `transform_gaussians(g, T)` with g a `Gaussians` (gaussian_adapter.Gaussians or any dataclass with its
    fields): returns a new one with means, world covariances [..., 3, 3] and harmonics [..., 3, d_sh] transformed, scales
    multiplied by s and opacities shared.  Its `rotations` are kept: the adapter's quaternions describe a Gaussian in the
    frame of its camera, which moves with the scene (transform_cameras).

    Tensor form, `transform_gaussians(None, T, means=, scales=, rotations=, covariances=, harmonics=)`: any subset; returns the
    tuple (means, scales, rotations, covariances, harmonics) with None where None went in.  rotations are world-frame
    quaternions in `quat_order` ("wxyz" as GaussianAdam and the rasterizer, or "xyzw"); covariances [..., 3, 3] or the six
    entries [..., 6]; harmonics in `sh_layout`.  All arrays share their leading shape.

    One or two library launches after the table's; differentiable with respect to every array given and to a device transform
    that requires grad (the module docstring; its backward adds the two launches of the tangent reduction)."""
    if transform is None:
        raise ValueError(f"{_P}transform_gaussians needs a transform")
    if gaussians is not None:
        if any(x is not None for x in (means, scales, rotations, covariances, harmonics)):
            raise ValueError(f"{_P}give either a Gaussians dataclass or tensors, not both")
        m, s, _, c, h = _apply(transform, gaussians.means, gaussians.scales, None, gaussians.covariances, gaussians.harmonics,
                               view_ids, "wxyz", "channel_major")
        return dataclasses.replace(gaussians, means=m, covariances=c, harmonics=h, scales=s)
    return _apply(transform, means, scales, rotations, covariances, harmonics, view_ids, quat_order, sh_layout)


def _apply(transform, means, scales, rotations, covariances, harmonics, view_ids, quat_order, sh_layout):
    if quat_order not in QUAT_ORDERS:
        raise ValueError(f"{_P}quat_order must be one of {QUAT_ORDERS}, got {quat_order!r}")
    if not any(_is_device(x) for x in (transform if isinstance(transform, (tuple, list)) else (transform,))):
        _split_host(transform)                # a host transform is judged first: its errors need no device
    flags, M, N, device = _array_layout(means, scales, rotations, covariances, harmonics, quat_order, sh_layout)
    xf, batched, live = _xf_live(transform, device)
    if live is not None and xf.shape[0] > _lib.SIM3_MAX_ROWS:
        raise ValueError(f"{_P}a transform that requires grad may have up to {_lib.SIM3_MAX_ROWS} rows, got {xf.shape[0]}")
    ids = _ids(view_ids, N, xf.shape[0], batched, device)
    return _Transform.apply(live, prepare_table(xf), ids, flags, M, N, means, scales, rotations, covariances, harmonics)


def _array_layout(means, scales, rotations, covariances, harmonics, quat_order, sh_layout) -> tuple:
    """(layout flags, M, N, device) of the arrays given (any subset; float32 device tensors that agree on N), after the checks."""
    if quat_order not in QUAT_ORDERS:
        raise ValueError(f"{_P}quat_order must be one of {QUAT_ORDERS}, got {quat_order!r}")
    given = [(n, t) for n, t in (("means", means), ("scales", scales), ("rotations", rotations), ("covariances", covariances),
                                 ("harmonics", harmonics)) if t is not None]
    if not given:
        raise ValueError(f"{_P}nothing to transform")
    for n, t in given:
        _f32(t, n)
    device = given[0][1].device
    if any(t.device != device for _, t in given):
        raise ValueError(f"{_P}tensors on different devices")
    flags, M, counts = 0, 1, {}
    for n, t, w in (("means", means, 3), ("scales", scales, 3), ("rotations", rotations, 4)):
        if t is not None:
            if t.dim() < 1 or t.shape[-1] != w:
                raise ValueError(f"{_P}{n} must be [..., {w}], got {tuple(t.shape)}")
            counts[n] = t.numel() // w
    if covariances is not None:
        if covariances.dim() >= 2 and tuple(covariances.shape[-2:]) == (3, 3):
            flags |= _lib.TRANSFORM_COV_FULL
            counts["covariances"] = covariances.numel() // 9
        elif covariances.shape[-1] == 6:
            counts["covariances"] = covariances.numel() // 6
        else:
            raise ValueError(f"{_P}covariances must be [..., 3, 3] or [..., 6], got {tuple(covariances.shape)}")
    if harmonics is not None:
        M, counts["harmonics"] = _sh_dims(harmonics, sh_layout)
        flags |= _lib.TRANSFORM_SH_CHANNEL_MAJOR if sh_layout == "channel_major" else 0
    if len(set(counts.values())) != 1:
        raise ValueError(f"{_P}the arrays disagree on the number of Gaussians: {counts}")
    if quat_order == "xyzw":
        flags |= _lib.TRANSFORM_QUAT_XYZW
    return flags, M, next(iter(counts.values())), device


# ---- helpers on transforms and cameras ----------------------------------------------------------------------------------------

def _parts(T):
    """(s [...], R [..., 3, 3], t [..., 3]) of a transform as tensors (float64 for host input, as given on the device)."""
    if isinstance(T, (tuple, list)) and len(T) == 3:
        dev = next((x.device for x in T if _is_device(x)), None)
        if dev is None:
            s, R, t = (_f64(x) for x in T)
        else:
            s, R, t = (torch.as_tensor(x, dtype=torch.float32, device=dev) if not isinstance(x, Tensor) else x.to(dev) for x in T)
        return s, R, t
    M = T if _is_device(T) else _f64(T)
    if tuple(M.shape[-2:]) not in ((4, 4), (3, 4)):
        raise ValueError(f"{_P}a transform is a 4 x 4 matrix or a tuple (s, R, t); got shape {tuple(M.shape)}")
    A = M[..., :3, :3]
    s = torch.linalg.det(A).abs().pow(1.0 / 3.0) * torch.sign(torch.linalg.det(A))
    return s, A / s[..., None, None], M[..., :3, 3]


def similarity_matrix(s, R, t) -> Tensor:
    """The 4 x 4 matrix [s R | t; 0 0 0 1] of (s, R, t)."""
    s, R, t = _parts((s, R, t))
    M = torch.zeros(R.shape[:-2] + (4, 4), dtype=R.dtype, device=R.device)
    M[..., :3, :3] = s[..., None, None] * R
    M[..., :3, 3] = t
    M[..., 3, 3] = 1.0
    return M


def similarity_inverse(T):
    """(s, R, t) of the inverse: x -> (1 / s) R^T (x - t).  Returns a 4 x 4 for a 4 x 4 and a tuple for a tuple."""
    s, R, t = _parts(T)
    si, Ri = 1.0 / s, R.transpose(-1, -2)
    ti = -(si[..., None] * torch.einsum("...ij,...j->...i", Ri, t))
    return (si, Ri, ti) if isinstance(T, (tuple, list)) else similarity_matrix(si, Ri, ti)


def compose(A, B):
    """The transform "B first, then A": x -> A(B(x)).  Returns a 4 x 4 if A is one, else a tuple (s, R, t)."""
    sa, Ra, ta = _parts(A)
    sb, Rb, tb = _parts(B)
    if Ra.device != Rb.device or Ra.dtype != Rb.dtype:
        sb, Rb, tb = (x.to(device=Ra.device, dtype=Ra.dtype) for x in (sb, Rb, tb))
    s, R = sa * sb, Ra @ Rb
    t = sa[..., None] * torch.einsum("...ij,...j->...i", Ra, tb) + ta
    return (s, R, t) if isinstance(A, (tuple, list)) else similarity_matrix(s, R, t)


def transform_cameras(extrinsics: Tensor, transform) -> Tensor:
    """Camera-to-world matrices [..., 4, 4] of the cameras that see the transformed scene as the given ones saw the original:
    the RIGID c2w' = [R R_c | s R c + t; 0 0 0 1] (the scale goes into the position only, so depths come out multiplied by s).
    Plain torch in the dtype and on the device of `extrinsics`."""
    if extrinsics.shape[-2:] != (4, 4):
        raise ValueError(f"{_P}extrinsics must be [..., 4, 4], got {tuple(extrinsics.shape)}")
    s, R, t = (x.to(device=extrinsics.device, dtype=extrinsics.dtype) for x in _parts(transform))
    out = extrinsics.clone()
    out[..., :3, :3] = R @ extrinsics[..., :3, :3]
    out[..., :3, 3] = s[..., None] * torch.einsum("...ij,...j->...i", R, extrinsics[..., :3, 3]) + t
    return out
