"""Torch restatement of freesplat_amd/depth_loss.py, written from the definitions (DESIGN.md "Depth loss") as NaN
PROPAGATION, the way the SimpleRecon-style losses read: an invalid ground-truth value becomes NaN, the blur pool is
F.conv2d(stride=2, padding=1), the Sobel pass F.pad(mode="replicate") + F.conv2d, and isfinite() of the ground truth's
gradients selects the elements.  Differentiable by autograd: float64 on the CPU as the reference, or float32 on a chosen device
as the eager yardstick (what a user would write without the fused path).

The kernels (csrc/depth_loss.hip) are written as masks on one residual pyramid instead; tests/test_depth_loss_host.py checks
the two formulations against each other.
"""
import math

import torch
import torch.nn.functional as F

MODES = ("log_l1", "l1")
DEFAULTS = dict(mode="log_l1", num_scales=4, min_depth=0.0, max_depth=math.inf, alpha_floor=1e-3)


def _blur_kernel(like):
    k = torch.tensor([1.0, 2.0, 1.0], dtype=like.dtype, device=like.device)
    return (k[:, None] * k[None, :] / 16.0).view(1, 1, 3, 3)


def _sobel_kernels(like):
    sx = torch.tensor([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]], dtype=like.dtype, device=like.device) / 8.0
    return torch.stack([sx, sx.t()]).view(2, 1, 3, 3)


def expected_depth(depth, alpha, alpha_floor):
    return depth if alpha is None else depth / alpha.clamp_min(alpha_floor)


def gt_with_nans(gt, min_depth, max_depth):
    valid = torch.isfinite(gt) & (gt > min_depth) & (gt < max_depth)
    return torch.where(valid, gt, torch.full_like(gt, float("nan")))


def pyramid(x, num_scales):
    """[B, H, W] -> list of num_scales levels [B, 1, H_s, W_s]."""
    levels = [x[:, None]]
    for _ in range(num_scales - 1):
        levels.append(F.conv2d(levels[-1], _blur_kernel(x), stride=2, padding=1))
    return levels


def spatial_gradient(x):
    """[B, 1, H, W] -> [B, 2, H, W]: (g_x, g_y), Sobel / 8 with replicate padding."""
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), _sobel_kernels(x))


def terms(depth, gt, alpha=None, *, mode="log_l1", num_scales=4, min_depth=0.0, max_depth=math.inf, alpha_floor=1e-3):
    """(point_sum [B], point_cnt [B], grad_sum [B, S], grad_cnt [B, S]) in the inputs' dtype."""
    if mode not in MODES:
        raise ValueError(mode)
    E = expected_depth(depth, alpha, alpha_floor)
    g = gt_with_nans(gt, min_depth, max_depth)
    if mode == "log_l1":
        sel = torch.isfinite(g) & (E > 0)
        err = (torch.log(torch.where(sel, E, torch.ones_like(E))) - torch.log(torch.where(sel, g, torch.ones_like(g)))).abs()
    else:
        sel = torch.isfinite(g)
        err = (E - torch.where(sel, g, torch.zeros_like(g))).abs()
    point_sum = torch.where(sel, err, torch.zeros_like(err)).flatten(1).sum(1)
    point_cnt = sel.flatten(1).sum(1).to(depth.dtype)
    grad_sum, grad_cnt = [], []
    for pe, pg in zip(pyramid(E, num_scales), pyramid(g, num_scales)):
        gg = spatial_gradient(pg)
        m = torch.isfinite(gg)
        diff = (spatial_gradient(pe) - torch.where(m, gg, torch.zeros_like(gg))).abs()
        grad_sum.append(torch.where(m, diff, torch.zeros_like(diff)).flatten(1).sum(1))
        grad_cnt.append(m.flatten(1).sum(1).to(depth.dtype))
    return point_sum, point_cnt, torch.stack(grad_sum, 1), torch.stack(grad_cnt, 1)


def abs_arguments(depth, gt, alpha=None, *, mode="log_l1", num_scales=4, min_depth=0.0, max_depth=math.inf, alpha_floor=1e-3):
    """The consumed arguments of every abs(), per term: [point, level 0, level 1, ...], each with the boolean set that
    selects them (same shapes).  What a test asserts its own inputs on: a sign that flips in fp32 is not an error."""
    E = expected_depth(depth, alpha, alpha_floor)
    g = gt_with_nans(gt, min_depth, max_depth)
    sel = torch.isfinite(g) & (E > 0) if mode == "log_l1" else torch.isfinite(g)
    if mode == "log_l1":
        arg = torch.log(torch.where(sel, E, torch.ones_like(E))) - torch.log(torch.where(sel, g, torch.ones_like(g)))
    else:
        arg = E - torch.where(sel, g, torch.zeros_like(g))
    out = [(arg, sel)]
    for pe, pg in zip(pyramid(E, num_scales), pyramid(g, num_scales)):
        gg = spatial_gradient(pg)
        m = torch.isfinite(gg)
        out.append((spatial_gradient(pe) - torch.where(m, gg, torch.zeros_like(gg)), m))
    return out


def combine(point_sum, point_cnt, grad_sum, grad_cnt, point_weight=1.0, grad_weight=1.0):
    """A term or level whose count is 0 contributes exactly 0 (a plain mean of an empty set would give NaN)."""
    pc, gc = point_cnt.sum(), grad_cnt.sum(0)
    point = torch.where(pc > 0, point_sum.sum() / pc.clamp_min(1.0), torch.zeros_like(pc))
    grad = torch.where(gc > 0, grad_sum.sum(0) / gc.clamp_min(1.0), torch.zeros_like(gc)).sum()
    return point_weight * point + grad_weight * grad


def depth_loss(depth, gt, alpha=None, *, point_weight=1.0, grad_weight=1.0, **kw):
    return combine(*terms(depth, gt, alpha, **kw), point_weight, grad_weight)


def _as(t, dtype, device):
    return None if t is None else torch.as_tensor(t).detach().to(device=device, dtype=dtype)


def values(depth, gt, alpha=None, dtype=torch.float64, device="cpu", **kw):
    """The four term tensors in `dtype` on `device`, no graph."""
    with torch.no_grad():
        return terms(_as(depth, dtype, device), _as(gt, dtype, device), _as(alpha, dtype, device), **kw)


def grad(depth, gt, alpha=None, g_point=None, g_grad=None, dtype=torch.float64, device="cpu", **kw):
    """autograd's d(sum_b g_point[b] point_sum[b] + sum_{b,s} g_grad[b,s] grad_sum[b,s]) / d(depth, alpha); a None
    cotangent leaves that term out.  -> (g_depth, g_alpha | None)."""
    d = _as(depth, dtype, device).requires_grad_(True)
    a = None if alpha is None else _as(alpha, dtype, device).requires_grad_(True)
    ps, _, gs, _ = terms(d, _as(gt, dtype, device), a, **kw)
    total = 0
    if g_point is not None:
        total = total + (ps * _as(g_point, dtype, device)).sum()
    if g_grad is not None:
        total = total + (gs * _as(g_grad, dtype, device)).sum()
    got = torch.autograd.grad(total, [d] if a is None else [d, a], allow_unused=True)
    z = lambda t, like: torch.zeros_like(like) if t is None else t
    return z(got[0], d), (None if a is None else z(got[1], a))


def loss_grad(depth, gt, alpha=None, dtype=torch.float64, device="cpu", point_weight=1.0, grad_weight=1.0, **kw):
    """(loss, g_depth, g_alpha | None) through the scalar loss."""
    d = _as(depth, dtype, device).requires_grad_(True)
    a = None if alpha is None else _as(alpha, dtype, device).requires_grad_(True)
    loss = depth_loss(d, _as(gt, dtype, device), a, point_weight=point_weight, grad_weight=grad_weight, **kw)
    if loss.grad_fn is None:
        return loss.detach(), torch.zeros_like(d), (None if a is None else torch.zeros_like(a))
    got = torch.autograd.grad(loss, [d] if a is None else [d, a], allow_unused=True)
    z = lambda t, like: torch.zeros_like(like) if t is None else t
    return loss.detach(), z(got[0], d), (None if a is None else z(got[1], a))
