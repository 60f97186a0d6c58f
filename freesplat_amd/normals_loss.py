"""Surface normals from depth and the cosine normals loss on the device, through fs_depth_normals_forward / _backward and
fs_normals_loss_forward / _backward (libfreesplat_hip.so, include/freesplat_amd_normals.h, csrc/normals_loss.hip).  The
definitions are those of DESIGN.md "Normals loss":

  E      = depth, or depth / max(alpha, alpha_floor) when the rasterizer's accumulated alpha is given; valid iff finite and > 0
  gt     valid iff isfinite(gt_depth) & (gt_depth > min_depth) & (gt_depth < max_depth)   (holes may be NaN, +-inf, 0, negative)
  S      = the separable 5 x 5 Gaussian blur of the depth (`smoothing` = sigma, replicate-clamped, valid iff all 25 taps are),
           or the depth itself (`smoothing=None`)
  P      = S(px, py) * ((px - cx) / fx, (py - cy) / fy, 1)
  n      = normalize(Sobel_x(P) / 8  x  Sobel_y(P) / 8), replicate-clamped, valid iff all nine taps are; a fronto-parallel
           plane gives (0, 0, +1), away from the camera
  t      = the same chain on gt_depth, or gt_normals as given (valid iff finite; not renormalised)
  loss   = sum over the pixels where n and t are valid of 0.5 (1 - n . t), / their number   (no such pixel: exactly 0)

`intrinsics` = (fx, fy, cx, cy) in pixels, [4] or [B, 4]; the caller folds its pixel-centre convention into cx, cy.  The
rasterizer's pixel p sees NDC (2 p + 1) / W - 1 (ndc2Pix), which is `intrinsics_from_fov`: fx = W / (2 tanfovx), cx = (W - 1) / 2.
The adapter's unprojection (gaussian_adapter.py) instead pairs INTEGER pixel coordinates with the dataset's K, whose principal
point is near W / 2: for normals that agree with its points pass K's own (fx, fy, cx, cy).

One forward and one backward library call per op; the loss never writes a normal map to memory.  For the backward nothing but
references to the inputs (depth, alpha, intrinsics, the target) is held: the backward recomputes the whole chain from them.
Under no_grad nothing is held at all.  Gradients go to `depth` and `alpha` only, deterministically (a gather, no atomics).
Device tensors only: there is no CPU / eager path.  The calls are capturable in a graph when `intrinsics` is a device tensor
(a host tensor or sequence is validated and copied to the device, which a capture does not allow).
"""
from __future__ import annotations

import math

import torch
from torch import Tensor

from . import _args, _lib

TILE_W, TILE_H = 32, 16   # pixels one workgroup owns (csrc/normals_loss.hip kTileW, kTileH); tests place shapes by it
HALO = 6                  # the backward's reach around a tile with smoothing (2 without)
_NAME = "freesplat_amd.normals_loss"


def intrinsics_from_fov(tanfovx: float, tanfovy: float, H: int, W: int):
    """(fx, fy, cx, cy) of the rasterizer's convention: pixel p is the ray through NDC (2 p + 1) / W - 1."""
    return W / (2.0 * tanfovx), H / (2.0 * tanfovy), (W - 1) / 2.0, (H - 1) / 2.0


def _intrinsics(intr, B: int, device) -> Tensor:
    """[B, 4] fp32 on `device`.  A device tensor is trusted (no host synchronisation); anything else is validated and copied."""
    if isinstance(intr, Tensor) and intr.device.type == "cuda":
        k = intr.detach().float()
        if k.device != device:
            raise ValueError("freesplat_amd.normals_loss: tensors on different devices")
    else:
        k = torch.as_tensor(intr, dtype=torch.float64)
        if k.shape[-1:] != (4,) or k.dim() not in (1, 2):
            raise ValueError(f"freesplat_amd.normals_loss: intrinsics must be [4] or [B, 4] = (fx, fy, cx, cy), got {tuple(k.shape)}")
        if not bool(torch.isfinite(k).all()) or not bool((k[..., :2] > 0).all()):
            raise ValueError("freesplat_amd.normals_loss: intrinsics must be finite with fx, fy > 0")
        k = k.float().to(device)
    if k.dim() == 1 and k.shape[0] == 4:
        k = k.expand(B, 4)
    if tuple(k.shape) != (B, 4):
        raise ValueError(f"freesplat_amd.normals_loss: intrinsics must be [4] or [{B}, 4] = (fx, fy, cx, cy), got {tuple(k.shape)}")
    return k.contiguous()


def _scalars(smoothing, min_depth, max_depth, alpha_floor):
    sigma = 0.0                                                   # the library's "no smoothing"
    if smoothing is not None:
        sigma = float(smoothing)
        if isinstance(smoothing, bool) or not (sigma > 0.0 and math.isfinite(sigma)):
            raise ValueError(f"freesplat_amd.normals_loss: smoothing must be None or a positive finite sigma, got {smoothing!r}")
    return (sigma, *_args.depth_scalars(min_depth, max_depth, alpha_floor, _NAME))


def _maps(depth, alpha, intrinsics):
    d, a = _args.depth_maps(_NAME, depth, alpha)
    return d, a, _intrinsics(intrinsics, d.shape[0], d.device)


class _DepthNormals(torch.autograd.Function):
    """depth, alpha | None [B, H, W], intrinsics [B, 4] -> normals [B, 3, H, W].  `pending` comes from the caller:
    torch.is_grad_enabled() is always False inside forward."""

    @staticmethod
    def forward(ctx, depth, alpha, intr, scalars, pending):
        B, H, W = depth.shape
        out = torch.empty(B, 3, H, W, device=depth.device)
        p = _lib.ptr
        _lib.launch("fs_depth_normals_forward", B, H, W, p(depth), p(alpha), p(intr), *scalars, p(out))
        ctx.scalars = scalars
        ctx.has_alpha = alpha is not None
        ctx.set_materialize_grads(False)
        if pending:
            ctx.save_for_backward(depth, intr) if alpha is None else ctx.save_for_backward(depth, intr, alpha)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        if g is None:
            return (None,) * 5
        depth, intr = ctx.saved_tensors[:2]
        alpha, (g,), g_depth, g_alpha = _args.backward_buffers(ctx, 2, g)
        B, H, W = depth.shape
        p = _lib.ptr
        _lib.launch("fs_depth_normals_backward", B, H, W, p(depth), p(alpha), p(intr), *ctx.scalars, p(g), p(g_depth), p(g_alpha))
        return g_depth, g_alpha, None, None, None


class _NormalsLoss(torch.autograd.Function):
    """depth, alpha | None, gt_depth | None [B, H, W], gt_normals | None [B, 3, H, W], intrinsics [B, 4] -> (sum [B], cnt [B])
    float64."""

    @staticmethod
    def forward(ctx, depth, alpha, intr, gt_depth, gt_normals, scalars, pending):
        B, H, W = depth.shape
        L = _lib.lib()
        dev = depth.device
        scratch = torch.empty(L.fs_normals_scratch_bytes(B, H, W), dtype=torch.uint8, device=dev)
        total, cnt = (torch.empty(B, dtype=torch.float64, device=dev) for _ in range(2))
        p = _lib.ptr
        _lib.launch("fs_normals_loss_forward", B, H, W, p(depth), p(alpha), p(intr), p(gt_depth), p(gt_normals), *scalars,
                    p(total), p(cnt), p(scratch))
        ctx.scalars = scalars
        ctx.has_alpha, ctx.from_depth = alpha is not None, gt_depth is not None
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(cnt)
        if pending:
            gt = gt_depth if gt_depth is not None else gt_normals
            ctx.save_for_backward(depth, intr, gt) if alpha is None else ctx.save_for_backward(depth, intr, gt, alpha)
        return total, cnt

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_sum, _g_cnt):
        if g_sum is None:
            return (None,) * 7
        depth, intr, gt = ctx.saved_tensors[:3]
        alpha, (g_sum,), g_depth, g_alpha = _args.backward_buffers(ctx, 3, g_sum)
        gt_depth, gt_normals = (gt, None) if ctx.from_depth else (None, gt)
        B, H, W = depth.shape
        p = _lib.ptr
        _lib.launch("fs_normals_loss_backward", B, H, W, p(depth), p(alpha), p(intr), p(gt_depth), p(gt_normals), *ctx.scalars,
                    p(g_sum), p(g_depth), p(g_alpha))
        return g_depth, g_alpha, None, None, None, None, None


def depth_normals(depth: Tensor, intrinsics, alpha: Tensor | None = None, *, smoothing: float | None = 2.0,
                  alpha_floor: float = 1e-3, min_depth: float = 0.0, max_depth: float = math.inf) -> Tensor:
    """Camera-space normals [B, 3, H, W] of a depth map, NaN in all three channels where invalid (here min_depth / max_depth
    apply to the depth itself).  Differentiable with respect to `depth` and `alpha`; the cotangent of an invalid pixel is
    ignored.  Use it under no_grad to precompute a sensor's normals once per view, or to look at a reconstruction."""
    scalars = _scalars(smoothing, min_depth, max_depth, alpha_floor)
    d, a, k = _maps(depth, alpha, intrinsics)
    return _DepthNormals.apply(d, a, k, scalars, _args.pending(d, a))


def normals_loss_terms(depth: Tensor, intrinsics, *, gt_depth: Tensor | None = None, gt_normals: Tensor | None = None,
                       alpha: Tensor | None = None, smoothing: float | None = 2.0, min_depth: float = 0.0,
                       max_depth: float = math.inf, alpha_floor: float = 1e-3):
    """(sum [B], cnt [B]) float64 from one library call; `sum` is differentiable with respect to `depth` and `alpha`.  Exactly
    one of gt_depth [B, H, W] (its normals come from the same chain, with min_depth / max_depth applied) and gt_normals
    [B, 3, H, W] is given."""
    scalars = _scalars(smoothing, min_depth, max_depth, alpha_floor)
    if (gt_depth is None) == (gt_normals is None):
        raise ValueError("freesplat_amd.normals_loss: exactly one of gt_depth and gt_normals must be given")
    gt = gt_depth if gt_depth is not None else gt_normals
    _args.no_grad_to(gt, "the target", _NAME)
    d, a, k = _maps(depth, alpha, intrinsics)
    g = _args.device_f32(gt, "gt_depth" if gt_depth is not None else "gt_normals", _NAME).detach()
    B, H, W = d.shape
    want = (B, H, W) if gt_depth is not None else (B, 3, H, W)
    if tuple(g.shape) != want:
        raise ValueError(f"freesplat_amd.normals_loss: the target must be {want} for a depth of {tuple(d.shape)}, got {tuple(g.shape)}")
    if g.device != d.device:
        raise ValueError("freesplat_amd.normals_loss: tensors on different devices")
    return _NormalsLoss.apply(d, a, k, g if gt_depth is not None else None, g if gt_depth is None else None, scalars, _args.pending(d, a))


def combine(total: Tensor, cnt: Tensor) -> Tensor:
    """sum_b sum / max(sum_b cnt, 1): a sum whose count is 0 is an exact 0 itself.  No host synchronisation."""
    return total.sum() / cnt.sum().clamp_min_(1.0)


def normals_loss(depth: Tensor, intrinsics, *, gt_depth: Tensor | None = None, gt_normals: Tensor | None = None,
                 alpha: Tensor | None = None, smoothing: float | None = 2.0, min_depth: float = 0.0, max_depth: float = math.inf,
                 alpha_floor: float = 1e-3) -> Tensor:
    """The scalar float32 loss: one forward and one backward library call."""
    return combine(*normals_loss_terms(depth, intrinsics, gt_depth=gt_depth, gt_normals=gt_normals, alpha=alpha, smoothing=smoothing,
                                       min_depth=min_depth, max_depth=max_depth, alpha_floor=alpha_floor)).float()
