"""Multi-view depth consistency and scale-invariant depth losses on the device, through fs_mv_depth_forward / _backward and
fs_si_depth_forward / _backward (libfreesplat_hip.so, include/freesplat_amd_mvdepth.h, csrc/mv_depth_loss.hip).  The
definitions are those of DESIGN.md "Multi-view depth loss":

  E      = depth, or depth / max(alpha, alpha_floor) when the rasterizer's accumulated alpha is given
  V0     = isfinite(gt) & (gt > min_depth) & (gt < max_depth); a source sample S is valid under the same three tests
           (holes may be NaN, +-inf, 0 or negative)
  pairs  [B, K, 3, 4] = [A | t] with M = K_s T_s<-w T_w<-c, A = M[:, :3] K_c^-1, t = M[:, 3]   (`pair_transforms`)
  q(D)   = D A (x, y, 1)^T + t for the integer pixel (x, y): the homogeneous source-image point of the pixel at depth D

  multi-view, per view b and source k:
    q = q(gt), z' = q[2] + 1e-8, (u, v) = (q[0], q[1]) / z' if |q[2]| > 1e-8 else (q[0], q[1])
    S = src[rint(v), rint(u)] (half to even), 0 outside the source map
    visible  = V0 & valid(S) & (z' > 0) & (z' < occlusion S)
    z_p'     = q(E)[2] + 1e-8, selected = visible & isfinite(z_p') & (z_p' > 0), r = log z_p' - log S
    sum[b,k] = sum over the selected pixels of |r|, cnt[b,k] = their number
  loss   = 1 / K sum_k (sum_b sum[b,k] / max(sum_b cnt[b,k], 1))

  scale-invariant, over P = V0 & isfinite(E) & (E > 0) with d = log gt - log E:
    s1[b] = sum d, s2[b] = sum d^2, n[b] = |P|
  loss   = sqrt(max(sum_b s2 / sum_b n - si_lambda (sum_b s1 / sum_b n)^2, 0)), 0 when no pixel is in P

`intrinsics` = (fx, fy, cx, cy) in pixels: the integer pixel (x, y) is the ray ((x - cx) / fx, (y - cy) / fy, 1) and a source
point projects to the integer pixel nearest to (fx X / Z + cx, fy Y / Z + cy); the caller folds its pixel-centre convention
into cx, cy (see normals_loss.py).

Sources come as src_depth [B, K, Hs, Ws], or as a pool [S, Hs, Ws] of resident sensor maps with src_index [B, K] int32 on the
device picking K of them per view; an index outside [0, S) makes its pair contribute nothing.  The indices stay on the device.

One forward and one backward library call per op.  For the backward nothing but references to the inputs is held: the
backward recomputes the gathers.  Under no_grad nothing is held at all.  Gradients go to `depth` and `alpha` only,
deterministically (a gather, no atomics); the gather location depends on `gt` alone and carries no gradient.  Device tensors
only: there is no CPU / eager path.  The calls are capturable in a graph.
"""
from __future__ import annotations

import math

import torch
from torch import Tensor

from . import _args, _lib

CHUNK = 1024              # pixels one workgroup owns (csrc/mv_depth_loss.hip kChunk); tests place shapes by it
MAX_SOURCES = _lib.MVDEPTH_MAX_SOURCES
_NAME = "freesplat_amd.mv_depth_loss"


def _scalars(min_depth, max_depth, alpha_floor, occlusion=None):
    scalars = _args.depth_scalars(min_depth, max_depth, alpha_floor, _NAME)
    if occlusion is None:
        return scalars
    occlusion = float(occlusion)
    if not (occlusion > 0.0 and math.isfinite(occlusion)):
        raise ValueError(f"{_NAME}: occlusion must be a positive finite factor, got {occlusion!r}")
    return (occlusion, *scalars)


def _maps(depth, gt, alpha):
    _args.no_grad_to(gt, "gt", _NAME)
    d, a, g = _args.depth_maps(_NAME, depth, alpha, gt)
    return d, g, a


def _sources(d: Tensor, src_depth, pairs, src_index):
    """-> (src [B, K, Hs, Ws] | [S, Hs, Ws], pairs [B, K, 3, 4], src_index [B, K] int32 | None, K, S_pool)."""
    _args.no_grad_to(src_depth, "src_depth", _NAME)
    B = d.shape[0]
    s = _args.device_f32(src_depth, "src_depth", _NAME).detach()
    q = _args.device_f32(pairs, "pairs", _NAME).detach()
    if q.dim() != 4 or q.shape[0] != B or tuple(q.shape[2:]) != (3, 4):
        raise ValueError(f"{_NAME}: pairs must be [{B}, K, 3, 4] (pair_transforms), got {tuple(q.shape)}")
    K = q.shape[1]
    if not 1 <= K <= MAX_SOURCES:
        raise ValueError(f"{_NAME}: the number of sources per view must be in 1..{MAX_SOURCES}, got {K}")
    idx, S_pool = None, 0
    if src_index is None:
        if s.dim() != 4 or tuple(s.shape[:2]) != (B, K):
            raise ValueError(f"{_NAME}: src_depth must be [{B}, {K}, Hs, Ws] without src_index, got {tuple(s.shape)}")
    else:
        if not isinstance(src_index, Tensor) or src_index.device.type != "cuda" or src_index.is_floating_point():
            raise ValueError(f"{_NAME}: src_index must be an integer tensor on a HIP device")
        idx = src_index.to(torch.int32).contiguous()           # (values beyond int32 would be out of range either way)
        if s.dim() != 3 or tuple(idx.shape) != (B, K):
            raise ValueError(f"{_NAME}: with src_index, src_depth must be a pool [S, Hs, Ws] and src_index [{B}, {K}], got "
                             f"{tuple(s.shape)} and {tuple(idx.shape)}")
        S_pool = s.shape[0]
        if idx.device != d.device:
            raise ValueError(f"{_NAME}: tensors on different devices")
    if s.numel() == 0:
        raise ValueError(f"{_NAME}: empty src_depth")
    if s.device != d.device or q.device != d.device:
        raise ValueError(f"{_NAME}: tensors on different devices")
    return s, q, idx, K, S_pool


def _intr(k, lead, what: str, dtype, device) -> Tensor:
    """(fx, fy, cx, cy) as [4] or [*lead, 4] -> [*lead, 4]."""
    k = torch.as_tensor(k).detach().to(device=device, dtype=dtype)
    if k.shape == (4,):
        k = k.expand(*lead, 4)
    if tuple(k.shape) != (*lead, 4):
        raise ValueError(f"{_NAME}: {what} must be [4] or {[*lead, 4]} = (fx, fy, cx, cy), got {tuple(k.shape)}")
    return k


def pair_transforms(intrinsics, cam_to_world: Tensor, src_intrinsics, src_world_to_cam: Tensor, src_index: Tensor | None = None) -> Tensor:
    """pairs [B, K, 3, 4] fp32 = [A | t] for every (view, source): M = K_s T_s<-w T_w<-c, A = M[:, :3] K_c^-1, t = M[:, 3].

    intrinsics [4] | [B, 4] and cam_to_world [B, 4, 4] of the current views; src_intrinsics [4] | [B, K, 4] and src_world_to_cam
    [B, K, 4, 4] of their sources, or pool-shaped [4] | [S, 4] and [S, 4, 4] with src_index [B, K] (an index out of range gives
    a pair the loss never reads).  A few tiny matmuls in float64 where cam_to_world lives, rounded once; no host
    synchronisation."""
    if not isinstance(cam_to_world, Tensor) or cam_to_world.dim() != 3 or tuple(cam_to_world.shape[1:]) != (4, 4):
        raise ValueError(f"{_NAME}: cam_to_world must be [B, 4, 4], got {tuple(getattr(cam_to_world, 'shape', ()))}")
    dev, f64 = cam_to_world.device, torch.float64
    B = cam_to_world.shape[0]
    c2w = cam_to_world.detach().to(f64)
    if not isinstance(src_world_to_cam, Tensor):
        raise ValueError(f"{_NAME}: src_world_to_cam must be a tensor")
    w2s = src_world_to_cam.detach().to(device=dev, dtype=f64)
    if src_index is None:
        if w2s.dim() != 4 or w2s.shape[0] != B or tuple(w2s.shape[2:]) != (4, 4):
            raise ValueError(f"{_NAME}: src_world_to_cam must be [{B}, K, 4, 4] without src_index, got {tuple(w2s.shape)}")
        ks = _intr(src_intrinsics, w2s.shape[:2], "src_intrinsics", f64, dev)
    else:
        if w2s.dim() != 3 or tuple(w2s.shape[1:]) != (4, 4) or w2s.shape[0] == 0:
            raise ValueError(f"{_NAME}: with src_index, src_world_to_cam must be a pool [S, 4, 4], got {tuple(w2s.shape)}")
        if not isinstance(src_index, Tensor) or src_index.is_floating_point() or src_index.dim() != 2 or src_index.shape[0] != B:
            raise ValueError(f"{_NAME}: src_index must be an integer tensor [{B}, K]")
        pick = src_index.to(device=dev, dtype=torch.long).clamp(0, w2s.shape[0] - 1)
        ks = _intr(src_intrinsics, (w2s.shape[0],), "src_intrinsics", f64, dev)[pick]
        w2s = w2s[pick]
    kc = _intr(intrinsics, (B,), "intrinsics", f64, dev)
    K = w2s.shape[1]
    Ks = torch.zeros(B, K, 3, 3, dtype=f64, device=dev)
    Ks[..., 0, 0], Ks[..., 1, 1], Ks[..., 0, 2], Ks[..., 1, 2], Ks[..., 2, 2] = ks[..., 0], ks[..., 1], ks[..., 2], ks[..., 3], 1.0
    Kc_inv = torch.zeros(B, 3, 3, dtype=f64, device=dev)
    Kc_inv[:, 0, 0], Kc_inv[:, 1, 1], Kc_inv[:, 2, 2] = 1.0 / kc[:, 0], 1.0 / kc[:, 1], 1.0
    Kc_inv[:, 0, 2], Kc_inv[:, 1, 2] = -kc[:, 2] / kc[:, 0], -kc[:, 3] / kc[:, 1]
    M = Ks @ (w2s @ c2w[:, None])[..., :3, :]
    return torch.cat([M[..., :3] @ Kc_inv[:, None], M[..., 3:]], -1).float()


def _launch_forward(depth, gt, alpha, src, idx, pairs, K, S_pool, scalars, residual):
    B, H, W = depth.shape
    Hs, Ws = src.shape[-2:]
    L = _lib.lib()
    dev = depth.device
    scratch = torch.empty(L.fs_mvdepth_scratch_bytes(B, K, H, W), dtype=torch.uint8, device=dev)
    total, cnt = (torch.empty(B, K, dtype=torch.float64, device=dev) for _ in range(2))
    p = _lib.ptr
    _lib.launch("fs_mv_depth_forward", B, K, H, W, Hs, Ws, S_pool, p(depth), p(gt), p(alpha), p(src), p(idx), p(pairs), *scalars,
                p(total), p(cnt), p(residual), p(scratch))
    return total, cnt


class _MVDepth(torch.autograd.Function):
    """depth, gt, alpha | None [B, H, W], src, src_index | None, pairs -> (sum [B, K], cnt [B, K]) float64.  `pending` comes from
    the caller: torch.is_grad_enabled() is always False inside forward."""

    @staticmethod
    def forward(ctx, depth, gt, alpha, src, idx, pairs, K, S_pool, scalars, pending):
        total, cnt = _launch_forward(depth, gt, alpha, src, idx, pairs, K, S_pool, scalars, None)
        ctx.args = (K, S_pool, scalars)
        ctx.has_alpha, ctx.has_index = alpha is not None, idx is not None
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(cnt)
        if pending:
            ctx.save_for_backward(*(t for t in (depth, gt, src, pairs, alpha, idx) if t is not None))
        return total, cnt

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_sum, _g_cnt):
        if g_sum is None:
            return (None,) * 10
        depth, gt, src, pairs = ctx.saved_tensors[:4]
        alpha, (g_sum,), g_depth, g_alpha = _args.backward_buffers(ctx, 4, g_sum)
        idx = ctx.saved_tensors[-1] if ctx.has_index else None
        K, S_pool, scalars = ctx.args
        B, H, W = depth.shape
        Hs, Ws = src.shape[-2:]
        p = _lib.ptr
        _lib.launch("fs_mv_depth_backward", B, K, H, W, Hs, Ws, S_pool, p(depth), p(gt), p(alpha), p(src), p(idx), p(pairs),
                    *scalars, p(g_sum), p(g_depth), p(g_alpha))
        return (g_depth, None, g_alpha) + (None,) * 7


class _SIDepth(torch.autograd.Function):
    """depth, gt, alpha | None [B, H, W] -> (s1 [B], s2 [B], n [B]) float64."""

    @staticmethod
    def forward(ctx, depth, gt, alpha, scalars, pending):
        B, H, W = depth.shape
        L = _lib.lib()
        dev = depth.device
        scratch = torch.empty(L.fs_mvdepth_scratch_bytes(B, 0, H, W), dtype=torch.uint8, device=dev)
        s1, s2, n = (torch.empty(B, dtype=torch.float64, device=dev) for _ in range(3))
        p = _lib.ptr
        _lib.launch("fs_si_depth_forward", B, H, W, p(depth), p(gt), p(alpha), *scalars, p(s1), p(s2), p(n), p(scratch))
        ctx.scalars = scalars
        ctx.has_alpha = alpha is not None
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(n)
        if pending:
            ctx.save_for_backward(depth, gt) if alpha is None else ctx.save_for_backward(depth, gt, alpha)
        return s1, s2, n

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_s1, g_s2, _g_n):
        if g_s1 is None and g_s2 is None:
            return (None,) * 5
        depth, gt = ctx.saved_tensors[:2]
        alpha, cots, g_depth, g_alpha = _args.backward_buffers(ctx, 2, g_s1, g_s2)
        B, H, W = depth.shape
        g_s1, g_s2 = (torch.zeros(B, device=depth.device) if g is None else g for g in cots)
        p = _lib.ptr
        _lib.launch("fs_si_depth_backward", B, H, W, p(depth), p(gt), p(alpha), *ctx.scalars, p(g_s1), p(g_s2), p(g_depth),
                    p(g_alpha))
        return g_depth, None, g_alpha, None, None


def mv_depth_terms(depth: Tensor, gt: Tensor, src_depth: Tensor, pairs: Tensor, alpha: Tensor | None = None, *,
                   src_index: Tensor | None = None, occlusion: float = 1.05, min_depth: float = 0.0, max_depth: float = math.inf,
                   alpha_floor: float = 1e-3):
    """(sum [B, K], cnt [B, K]) float64 from one library call; `sum` is differentiable with respect to `depth` and `alpha`."""
    scalars = _scalars(min_depth, max_depth, alpha_floor, occlusion)
    d, g, a = _maps(depth, gt, alpha)
    s, q, idx, K, S_pool = _sources(d, src_depth, pairs, src_index)
    return _MVDepth.apply(d, g, a, s, idx, q, K, S_pool, scalars, _args.pending(d, a))


def combine(total: Tensor, cnt: Tensor) -> Tensor:
    """1 / K sum_k (sum_b sum[b,k] / max(sum_b cnt[b,k], 1)): the batch is pooled per source index, a source column without a
    selected pixel contributes exactly 0 (its sum is an exact 0 itself).  No host synchronisation."""
    return (total.sum(0) / cnt.sum(0).clamp_min_(1.0)).mean()


def mv_depth_loss(depth: Tensor, gt: Tensor, src_depth: Tensor, pairs: Tensor, alpha: Tensor | None = None, *,
                  src_index: Tensor | None = None, occlusion: float = 1.05, min_depth: float = 0.0, max_depth: float = math.inf,
                  alpha_floor: float = 1e-3) -> Tensor:
    """The scalar float32 loss: one forward and one backward library call."""
    return combine(*mv_depth_terms(depth, gt, src_depth, pairs, alpha, src_index=src_index, occlusion=occlusion,
                                   min_depth=min_depth, max_depth=max_depth, alpha_floor=alpha_floor)).float()


def mv_depth_residuals(depth: Tensor, gt: Tensor, src_depth: Tensor, pairs: Tensor, alpha: Tensor | None = None, *,
                       src_index: Tensor | None = None, occlusion: float = 1.05, min_depth: float = 0.0,
                       max_depth: float = math.inf, alpha_floor: float = 1e-3) -> Tensor:
    """The signed residuals r = log z_p' - log S [B, K, H, W], NaN where a pixel is not selected for a source: which pixels
    disagree with which neighbour.  Forward only, detached."""
    scalars = _scalars(min_depth, max_depth, alpha_floor, occlusion)
    d, g, a = _maps(depth, gt, alpha)
    s, q, idx, K, S_pool = _sources(d, src_depth, pairs, src_index)
    B, H, W = d.shape
    residual = torch.empty(B, K, H, W, device=d.device)
    _launch_forward(d, g, a, s, idx, q, K, S_pool, scalars, residual)            # (pointers only: no graph is recorded)
    return residual


def si_depth_terms(depth: Tensor, gt: Tensor, alpha: Tensor | None = None, *, min_depth: float = 0.0, max_depth: float = math.inf,
                   alpha_floor: float = 1e-3):
    """(s1 [B], s2 [B], n [B]) float64 from one library call; s1 and s2 are differentiable with respect to `depth` and `alpha`."""
    scalars = _scalars(min_depth, max_depth, alpha_floor)
    d, g, a = _maps(depth, gt, alpha)
    return _SIDepth.apply(d, g, a, scalars, _args.pending(d, a))


def combine_si(s1: Tensor, s2: Tensor, n: Tensor, si_lambda: float = 0.85) -> Tensor:
    """sqrt(max(sum s2 / N - si_lambda (sum s1 / N)^2, 0)) with N = sum n; exactly 0 (value and gradient) when N = 0 or the
    radicand is not positive.  No host synchronisation."""
    N = n.sum().clamp_min_(1.0)
    mean = s1.sum() / N
    var = s2.sum() / N - si_lambda * mean * mean
    pos = var > 0
    return torch.where(pos, torch.where(pos, var, torch.ones_like(var)).sqrt(), torch.zeros_like(var))


def scale_invariant_loss(depth: Tensor, gt: Tensor, alpha: Tensor | None = None, *, si_lambda: float = 0.85, min_depth: float = 0.0,
                         max_depth: float = math.inf, alpha_floor: float = 1e-3) -> Tensor:
    """The scalar float32 loss of Eigen et al. against a depth whose scale is unknown (si_lambda = 1: fully scale-invariant)."""
    si_lambda = float(si_lambda)
    if not math.isfinite(si_lambda):
        raise ValueError(f"{_NAME}: si_lambda must be finite, got {si_lambda!r}")
    return combine_si(*si_depth_terms(depth, gt, alpha, min_depth=min_depth, max_depth=max_depth, alpha_floor=alpha_floor),
                      si_lambda).float()
