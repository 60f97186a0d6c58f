"""Depth supervision on the device: a log-L1 (or L1) point term and a multi-scale gradient term over a blur-pool pyramid,
through fs_depth_loss_forward / fs_depth_loss_backward (libfreesplat_hip.so, include/freesplat_amd_depthloss.h,
csrc/depth_loss.hip).  The definitions are those of DESIGN.md "Depth loss":

  E      = depth, or depth / max(alpha, alpha_floor) when the rasterizer's accumulated alpha is given
  V0     = isfinite(gt) & (gt > min_depth) & (gt < max_depth)        (holes may be NaN, +-inf, 0 or negative)
  point  = sum_P |log E - log gt| / |P|, P = V0 & (E > 0)            ("log_l1"), or sum_V0 |E - gt| / |V0| ("l1")
  grad   = sum over num_scales levels of the mean of |g_x(E) - g_x(gt)| and |g_y(E) - g_y(gt)| over the elements all of whose
           nine taps are valid: Sobel / 8 with replicate clamping, on a (1,2,1) x (1,2,1) / 16 stride-2 zero-padded pyramid
  loss   = point_weight * point + grad_weight * grad                 (a term or level without a valid element contributes 0)

One forward library call gives the per-view sums and counts; one backward call gives the gradients with respect to `depth`
and `alpha`, deterministically (a gather, no atomics).  `gt` gets no gradient.  For the backward the forward keeps levels
1.. of the residual pyramid (`saved_bytes`, about 1.33 bytes per pixel); without a pending backward nothing is kept.
Device tensors only: there is no CPU / eager path.
"""
from __future__ import annotations

import math

import torch
from torch import Tensor

from . import _args, _lib

TILE_W, TILE_H = 64, 32   # pixels of level 0 one workgroup owns (csrc/depth_loss.hip kTileW, kTileH); tests place shapes by it
UPPER_TILE_H = 8          # ... and TILE_W x UPPER_TILE_H elements of a level above (kUpperTileH)
MAX_SCALES = _lib.DEPTH_LOSS_MAX_SCALES
MODES = {"log_l1": _lib.DEPTH_LOSS_LOG_L1, "l1": _lib.DEPTH_LOSS_L1}
_NAME = "freesplat_amd.depth_loss"


def _mode(mode: str) -> int:
    if mode not in MODES:
        raise ValueError(f"freesplat_amd.depth_loss: mode must be one of {sorted(MODES)}, got {mode!r}")
    return MODES[mode]


def _scales(num_scales) -> int:
    if isinstance(num_scales, bool) or not isinstance(num_scales, int) or not 1 <= num_scales <= MAX_SCALES:
        raise ValueError(f"freesplat_amd.depth_loss: num_scales must be an integer in 1..{MAX_SCALES}, got {num_scales!r}")
    return num_scales


def _maps(depth: Tensor, gt: Tensor, alpha, mode: str, num_scales, min_depth, max_depth, alpha_floor):
    flags, S = _mode(mode), _scales(num_scales)
    scalars = _args.depth_scalars(min_depth, max_depth, alpha_floor, _NAME)
    _args.no_grad_to(gt, "gt", _NAME)
    d, a, g = _args.depth_maps(_NAME, depth, alpha, gt)
    return d, g, a, flags, S, scalars


def saved_bytes(B: int, H: int, W: int, num_scales: int = 4) -> int:
    """Bytes the forward keeps for a pending backward (levels 1.. of the fp32 residual pyramid)."""
    return int(_lib.lib().fs_depth_loss_saved_bytes(B, H, W, _scales(num_scales)))


class _DepthLoss(torch.autograd.Function):
    """depth, gt, alpha | None [B, H, W] -> (point_sum [B], point_cnt [B], grad_sum [B, S], grad_cnt [B, S]) float64.  `saved` is
    allocated by the caller (None: no backward is pending): torch.is_grad_enabled() is always False inside forward."""

    @staticmethod
    def forward(ctx, depth, gt, alpha, saved, flags, S, scalars):
        B, H, W = depth.shape
        L = _lib.lib()
        dev = depth.device
        scratch = torch.empty(L.fs_depth_loss_scratch_bytes(B, H, W, S), dtype=torch.uint8, device=dev)
        point_sum, point_cnt = (torch.empty(B, dtype=torch.float64, device=dev) for _ in range(2))
        grad_sum, grad_cnt = (torch.empty(B, S, dtype=torch.float64, device=dev) for _ in range(2))
        p = _lib.ptr
        _lib.launch("fs_depth_loss_forward", B, H, W, S, flags, p(depth), p(gt), p(alpha), *scalars, p(point_sum), p(point_cnt),
                    p(grad_sum), p(grad_cnt), p(saved), p(scratch))
        ctx.args = (flags, S, scalars)
        ctx.has_alpha = alpha is not None
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(point_cnt, grad_cnt)
        if saved is not None:
            ctx.save_for_backward(depth, gt, saved) if alpha is None else ctx.save_for_backward(depth, gt, saved, alpha)
        return point_sum, point_cnt, grad_sum, grad_cnt

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_point, _g_point_cnt, g_grad, _g_grad_cnt):
        if g_point is None and g_grad is None:
            return (None,) * 7
        depth, gt, saved = ctx.saved_tensors[:3]
        alpha, (g_point, g_grad), g_depth, g_alpha = _args.backward_buffers(ctx, 3, g_point, g_grad)
        flags, S, scalars = ctx.args
        B, H, W = depth.shape
        L = _lib.lib()
        scratch = torch.empty(L.fs_depth_loss_scratch_bytes(B, H, W, S), dtype=torch.uint8, device=depth.device)
        p = _lib.ptr
        _lib.launch("fs_depth_loss_backward", B, H, W, S, flags, p(depth), p(gt), p(alpha), *scalars, p(g_point), p(g_grad),
                    p(saved), p(g_depth), p(g_alpha), p(scratch))
        return g_depth, None, g_alpha, None, None, None, None


def depth_loss_terms(depth: Tensor, gt: Tensor, alpha: Tensor | None = None, *, mode: str = "log_l1", num_scales: int = 4,
                     min_depth: float = 0.0, max_depth: float = math.inf, alpha_floor: float = 1e-3):
    """(point_sum [B], point_cnt [B], grad_sum [B, S], grad_cnt [B, S]) float64 from one library call; the two sums are
    differentiable with respect to `depth` and `alpha`."""
    d, g, a, flags, S, scalars = _maps(depth, gt, alpha, mode, num_scales, min_depth, max_depth, alpha_floor)
    saved = None
    if _args.pending(d, a):
        B, H, W = d.shape
        saved = torch.empty(_lib.lib().fs_depth_loss_saved_bytes(B, H, W, S) // 4, device=d.device)
    return _DepthLoss.apply(d, g, a, saved, flags, S, scalars)


def combine(point_sum: Tensor, point_cnt: Tensor, grad_sum: Tensor, grad_cnt: Tensor, point_weight: float = 1.0,
            grad_weight: float = 1.0) -> Tensor:
    """point_weight * sum_b point_sum / sum_b point_cnt + grad_weight * sum_s (sum_b grad_sum / sum_b grad_cnt); a term or
    level whose count is 0 contributes exactly 0.  A few operations on [B] / [B, S] tensors, no host synchronisation."""
    # (a sum whose count is 0 is an exact 0 itself, so 0 / max(0, 1) needs no mask)
    point = point_sum.sum() / point_cnt.sum().clamp_min_(1.0)
    grad = (grad_sum.sum(0) / grad_cnt.sum(0).clamp_min_(1.0)).sum()
    if point_weight != 1.0:
        point = point_weight * point
    if grad_weight != 1.0:
        grad = grad_weight * grad
    return point + grad


def depth_loss(depth: Tensor, gt: Tensor, alpha: Tensor | None = None, *, mode: str = "log_l1", num_scales: int = 4,
               point_weight: float = 1.0, grad_weight: float = 1.0, min_depth: float = 0.0, max_depth: float = math.inf,
               alpha_floor: float = 1e-3) -> Tensor:
    """The scalar float32 loss: one forward and one backward library call for both terms."""
    terms = depth_loss_terms(depth, gt, alpha, mode=mode, num_scales=num_scales, min_depth=min_depth, max_depth=max_depth,
                             alpha_floor=alpha_floor)
    return combine(*terms, point_weight, grad_weight).float()
