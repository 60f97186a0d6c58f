"""Argument handling the fused ops share (depth_loss, normals_loss, mv_depth_loss, ssim_loss, lpips, metrics, refine).

Every function takes `name`, the calling module's "freesplat_amd.<module>": it prefixes the error messages, which the host
tests match verbatim.  A new op calls these instead of copying another module's checks.
"""
from __future__ import annotations

import math

import torch
from torch import Tensor


def device_tensor(t, what: str, name: str) -> Tensor:
    if not isinstance(t, Tensor) or t.device.type != "cuda":
        raise ValueError(f"{name}: {what} must be a tensor on a HIP device (got {getattr(t, 'device', type(t))}); "
                         "there is no CPU path")
    return t


def device_f32(t, what: str, name: str) -> Tensor:
    return device_tensor(t, what, name).float().contiguous()


def depth_scalars(min_depth, max_depth, alpha_floor, name: str):
    """(min_depth, max_depth, alpha_floor) as floats: no NaN bound, a positive finite floor."""
    min_depth, max_depth, alpha_floor = float(min_depth), float(max_depth), float(alpha_floor)
    if math.isnan(min_depth) or math.isnan(max_depth):
        raise ValueError(f"{name}: min_depth / max_depth must not be NaN")
    if not (alpha_floor > 0.0 and math.isfinite(alpha_floor)):
        raise ValueError(f"{name}: alpha_floor must be a positive finite number, got {alpha_floor!r}")
    return min_depth, max_depth, alpha_floor


def no_grad_to(t, what: str, name: str) -> None:
    if isinstance(t, Tensor) and t.requires_grad and torch.is_grad_enabled():
        raise RuntimeError(f"{name}: {what} gets no gradient from the fused loss; detach it (only `depth` and `alpha` are "
                           "differentiated)")


def depth_maps(name: str, depth, alpha, *gt):
    """depth, alpha | None and at most one target map `gt` as contiguous fp32 [B, H, W] device tensors of one shape on one
    device, the target detached -> (depth, alpha, *gt)."""
    d = device_f32(depth, "depth", name)
    g = [device_f32(t, "gt", name).detach() for t in gt]
    a = None if alpha is None else device_f32(alpha, "alpha", name)
    if d.dim() != 3 or any(t.shape != d.shape for t in g) or (a is not None and a.shape != d.shape):
        raise ValueError(f"{name}: expected [B, H, W] tensors of one shape, got " + ", ".join(str(tuple(t.shape)) for t in (d, *g))
                         + ("" if a is None else f" and {tuple(a.shape)}"))
    if any(t.device != d.device for t in g) or (a is not None and a.device != d.device):
        raise ValueError(f"{name}: tensors on different devices")
    if d.numel() == 0:
        raise ValueError(f"{name}: empty batch")
    return (d, a, *g)


def pending(d: Tensor, a) -> bool:
    """Whether a backward may follow: the caller asks, since torch.is_grad_enabled() is always False inside forward."""
    return torch.is_grad_enabled() and (d.requires_grad or (a is not None and a.requires_grad))


def backward_buffers(ctx, n_saved: int, *cotangents):
    """The opening of a depth-family backward.  ctx.saved_tensors = (depth, ... n_saved tensors ..., alpha when ctx.has_alpha,
    ...) -> (alpha | None, the cotangents as contiguous fp32 (None stays None), g_depth, g_alpha | None)."""
    depth = ctx.saved_tensors[0]
    alpha = ctx.saved_tensors[n_saved] if ctx.has_alpha else None
    cots = tuple(None if g is None else g.float().contiguous() for g in cotangents)
    g_depth = torch.empty(depth.shape, device=depth.device)
    g_alpha = None if alpha is None else torch.empty(depth.shape, device=depth.device)
    return alpha, cots, g_depth, g_alpha
