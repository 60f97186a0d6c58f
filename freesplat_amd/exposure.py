"""Per-view exposure compensation on the device, through fs_exposure_apply_forward / _backward and fs_exposure_fit
(libfreesplat_hip.so, include/freesplat_amd_exposure.h, csrc/exposure.hip).  The definitions are those of DESIGN.md
"Exposure compensation":

  params [V, 3, 4]   row c of view v is (A[c,0], A[c,1], A[c,2], b[c]); the identity is [I | 0]
  view_ids [B]       the view of each batch entry; None: B == V and entry b uses view b
  apply              out[b, c] = A[v,c,0] x0 + A[v,c,1] x1 + A[v,c,2] x2 + b[v,c], v = view_ids[b]; no clamp, no mask; an entry
                     whose id lies outside [0, V) passes through unchanged and contributes to no parameter gradient
  fit                per view, the affine map that takes `pred` to `target` in the least-squares sense over the valid pixels (mask
                     nonzero, all six colour values finite) of the entries with that id, pulled towards the identity by
                     `ridge`: P solves (M + ridge cnt I) P = R + ridge cnt [I; 0], M = sum X X^T, R = sum X y^T, X = (x, 1)

`apply_exposure` sits between the rasterizer's colour output and `photometric_loss`; `color_corrected` aligns a prediction to
its ground truth before `metrics.image_metrics` / `compute_psnr` for colour-corrected PSNR / SSIM.  One library call per op
and direction; every sum is fp64 in a fixed order without float atomics, so all results are bit-reproducible across runs,
streams, batch compositions and alignments.  For the backward only references to the inputs are held, and nothing at all under
no_grad.  Device tensors only: there is no CPU / eager path.  `view_ids` on the device are never read by the host (no
synchronisation, capturable in a graph); given as a Python sequence or a CPU tensor they are range-checked on the host.
"""
from __future__ import annotations

import math

import torch
from torch import Tensor, nn

from . import _lib

CHUNK = 4096   # pixels of one batch entry a workgroup owns (csrc/exposure.hip kChunk); tests place shapes by it
_P = "freesplat_amd.exposure: "


def _image(t, what: str) -> Tensor:
    if not isinstance(t, Tensor) or t.device.type != "cuda":
        raise ValueError(f"{_P}{what} must be a tensor on a HIP device (got {getattr(t, 'device', type(t))}); there is no CPU path")
    if t.dtype != torch.float32:
        raise ValueError(f"{_P}{what} must be float32, got {t.dtype}")
    if t.dim() != 4 or t.shape[1] != 3:
        raise ValueError(f"{_P}{what} must be [B, 3, H, W], got {tuple(t.shape)}")
    if t.numel() == 0:
        raise ValueError(f"{_P}{what} is empty: {tuple(t.shape)}")
    return t.contiguous()


def _params(p, device) -> Tensor:
    if not isinstance(p, Tensor) or p.device.type != "cuda":
        raise ValueError(f"{_P}params must be a tensor on a HIP device (got {getattr(p, 'device', type(p))}); there is no CPU path")
    if p.dtype != torch.float32:
        raise ValueError(f"{_P}params must be float32, got {p.dtype}")
    if p.dim() != 3 or tuple(p.shape[1:]) != (3, 4) or p.shape[0] == 0:
        raise ValueError(f"{_P}params must be [V, 3, 4] with V >= 1, got {tuple(p.shape)}")
    if p.device != device:
        raise ValueError(f"{_P}tensors on different devices")
    return p.contiguous()


def _view_ids(ids, B: int, V: int, device):
    """None, or [B] int64 on `device`.  A device tensor is trusted (the kernels pass an out-of-range entry through); anything
    else is range-checked here and copied."""
    if ids is None:
        if B != V:
            raise ValueError(f"{_P}without view_ids the batch must have one entry per view: B = {B}, V = {V}")
        return None
    if isinstance(ids, Tensor) and ids.device.type == "cuda":
        if ids.device != device:
            raise ValueError(f"{_P}tensors on different devices")
        if ids.dtype.is_floating_point or ids.dtype.is_complex or ids.dtype == torch.bool:
            raise ValueError(f"{_P}view_ids must be integers, got {ids.dtype}")
        if tuple(ids.shape) != (B,):
            raise ValueError(f"{_P}view_ids must be [{B}], got {tuple(ids.shape)}")
        return ids.detach().to(torch.int64).contiguous()
    host = torch.as_tensor(ids)
    if host.dtype.is_floating_point or host.dtype.is_complex or host.dtype == torch.bool:
        raise ValueError(f"{_P}view_ids must be integers, got {host.dtype}")
    if tuple(host.shape) != (B,):
        raise ValueError(f"{_P}view_ids must be [{B}], got {tuple(host.shape)}")
    host = host.to(torch.int64)
    if bool(((host < 0) | (host >= V)).any()):
        raise ValueError(f"{_P}view_ids must lie in [0, {V}), got {host.tolist()}")
    return host.to(device)


def _ridge(ridge) -> float:
    r = float(ridge)
    if isinstance(ridge, bool) or not (r >= 0.0 and math.isfinite(r)):
        raise ValueError(f"{_P}ridge must be a finite number >= 0, got {ridge!r}")
    return r


class _Apply(torch.autograd.Function):
    """image [B, 3, H, W], params [V, 3, 4], view_ids [B] int64 | None -> out [B, 3, H, W].  `pending` comes from the caller:
    torch.is_grad_enabled() is always False inside forward."""

    @staticmethod
    def forward(ctx, image, params, ids, pending):
        B, _, H, W = image.shape
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=image.device)
        p = _lib.ptr
        _lib.launch("fs_exposure_apply_forward", B, params.shape[0], H, W, p(image), p(params), p(ids), p(out))
        ctx.set_materialize_grads(False)
        ctx.has_ids = ids is not None
        ctx.dims = (B, params.shape[0], H, W)
        if pending:
            # the image is needed for g_params only; g_image needs the parameters and the cotangent
            keep = [params] + ([ids] if ids is not None else []) + ([image] if ctx.needs_input_grad[1] else [])
            ctx.save_for_backward(*keep)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None:
            return None, None, None, None
        want_image, want_params = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        saved = list(ctx.saved_tensors)
        params = saved.pop(0)
        ids = saved.pop(0) if ctx.has_ids else None
        image = saved.pop(0) if want_params else None
        B, V, H, W = ctx.dims
        if g.dtype != torch.float32:
            g = g.float()
        g = g.contiguous()
        L, dev = _lib.lib(), g.device
        g_image = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev) if want_image else None
        g_params = torch.empty(V, 3, 4, dtype=torch.float32, device=dev) if want_params else None
        scratch = torch.empty(L.fs_exposure_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev) if want_params else None
        p = _lib.ptr
        _lib.launch("fs_exposure_apply_backward", B, V, H, W, p(image), p(params), p(ids), p(g), p(g_image), p(g_params),
                    p(scratch))
        return g_image, g_params, None, None


def apply_exposure(image: Tensor, params: Tensor, view_ids=None) -> Tensor:
    """out[b] = A[v] image[b] + b[v] per pixel, v = view_ids[b] (None: v = b and B == V).  Differentiable with respect to `image`
    and `params`; only the gradients somebody asks for are computed."""
    x = _image(image, "image")
    q = _params(params, x.device)
    ids = _view_ids(view_ids, x.shape[0], q.shape[0], x.device)
    pending = torch.is_grad_enabled() and (x.requires_grad or q.requires_grad)
    return _Apply.apply(x, q, ids, pending)


def _mask(mask, B: int, H: int, W: int, device):
    """None, or [B, H, W] uint8 on `device`, nonzero = use."""
    if mask is None:
        return None
    if not isinstance(mask, Tensor) or mask.device.type != "cuda":
        raise ValueError(f"{_P}mask must be a tensor on a HIP device (got {getattr(mask, 'device', type(mask))}); there is no CPU path")
    if mask.device != device:
        raise ValueError(f"{_P}tensors on different devices")
    if tuple(mask.shape) != (B, H, W):
        raise ValueError(f"{_P}mask must be [{B}, {H}, {W}], got {tuple(mask.shape)}")
    if mask.dtype == torch.bool:
        return mask.contiguous().view(torch.uint8)
    if mask.dtype == torch.uint8:
        return mask.contiguous()
    return (mask != 0).contiguous().view(torch.uint8)


def fit_exposure(pred: Tensor, target: Tensor, mask: Tensor | None = None, view_ids=None, num_views: int | None = None,
                 ridge: float = 1e-6):
    """(params [V, 3, 4] float32, count [V] int64, solved [V] bool): per view the least-squares affine colour map from `pred` to
    `target` over the valid pixels of the entries with that id.  A view without a valid pixel (or, with ridge = 0, with a
    singular system) gets the identity exactly and solved = False.  No autograd: the inputs are taken as constants.
    `num_views` is required with device `view_ids` (the host never reads them); with host ids it defaults to max(id) + 1."""
    r = _ridge(ridge)
    x, y = _image(pred, "pred").detach(), _image(target, "target").detach()
    if x.shape != y.shape:
        raise ValueError(f"{_P}pred and target must have one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.device != y.device:
        raise ValueError(f"{_P}tensors on different devices")
    B, _, H, W = x.shape
    if num_views is None:
        if view_ids is None:
            V = B
        elif isinstance(view_ids, Tensor) and view_ids.device.type == "cuda":
            raise ValueError(f"{_P}num_views is required when view_ids live on the device")
        else:
            host = torch.as_tensor(view_ids)
            V = int(host.max()) + 1 if host.numel() and not host.dtype.is_floating_point else 0
    else:
        V = int(num_views)
    if V < 1:
        raise ValueError(f"{_P}num_views must be >= 1, got {V}")
    ids = _view_ids(view_ids, B, V, x.device)
    m = _mask(mask, B, H, W, x.device)
    L, dev = _lib.lib(), x.device
    params = torch.empty(V, 3, 4, dtype=torch.float32, device=dev)
    count = torch.empty(V, dtype=torch.int64, device=dev)
    solved = torch.empty(V, dtype=torch.uint8, device=dev)
    scratch = torch.empty(L.fs_exposure_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    _lib.launch("fs_exposure_fit", B, V, H, W, p(x), p(y), p(m), p(ids), r, p(params), p(count), p(solved), p(scratch))
    return params, count, solved.view(torch.bool)


def color_corrected(pred: Tensor, target: Tensor, mask: Tensor | None = None, ridge: float = 1e-6) -> Tensor:
    """`pred` aligned to its own ground truth per image: fit_exposure, then apply_exposure, under no_grad.  Feed the result to
    metrics.image_metrics / compute_psnr for colour-corrected metrics."""
    with torch.no_grad():
        params, _, _ = fit_exposure(pred, target, mask, ridge=ridge)
        return apply_exposure(pred.detach(), params)


class Exposure(nn.Module):
    """One affine colour transform per captured view, `params` [V, 3, 4] at the identity.  forward(image, view_ids) is
    apply_exposure; put it between the rasterizer's colour output and photometric_loss.

    Training: the 12 V floats are an ordinary nn.Parameter, stepped beside the Gaussians' own optimizer,

        gaussians = GaussianAdam(...)
        exposure = Exposure(num_views).to(device)
        exposure_opt = torch.optim.Adam([exposure.params], lr=1e-3)
        ...
        loss = photometric_loss(exposure(color, view_ids), gt, ...)
        loss.backward(); gaussians.step(); exposure_opt.step(); exposure_opt.zero_grad()

    (12 V floats do not warrant a kernel of their own).  fit_() initialises or resets views in closed form."""

    def __init__(self, num_views: int):
        super().__init__()
        if int(num_views) < 1:
            raise ValueError(f"{_P}num_views must be >= 1, got {num_views}")
        eye = torch.cat([torch.eye(3), torch.zeros(3, 1)], 1)
        self.params = nn.Parameter(eye.repeat(int(num_views), 1, 1))

    def forward(self, image: Tensor, view_ids=None) -> Tensor:
        return apply_exposure(image, self.params, view_ids)

    @torch.no_grad()
    def fit_(self, pred: Tensor, target: Tensor, mask: Tensor | None = None, view_ids=None, ridge: float = 1e-6) -> Tensor:
        """Overwrites, in place, the rows of the views that the fit solved; returns count [V]."""
        fitted, count, solved = fit_exposure(pred, target, mask, view_ids, self.params.shape[0], ridge)
        self.params.copy_(torch.where(solved.view(-1, 1, 1), fitted, self.params))
        return count
