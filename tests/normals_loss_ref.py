"""Torch restatement of freesplat_amd/normals_loss.py, written from the definitions (DESIGN.md "Normals loss") as NaN
PROPAGATION: an invalid depth becomes NaN, the 5 x 5 blur is plain arithmetic on clamped taps (it has no zero weight, so a NaN
tap makes a NaN output), and the nine-tap validity of a normal is isfinite() of the sum of its taps.  Before the non-linear steps
(points, cross product, normalise) a NaN is replaced by 1 under torch.where, so that autograd never multiplies a zero cotangent
with a NaN.  Differentiable by autograd: float64 on the CPU as the reference, or float32 on a chosen device as the eager yardstick
(what a user would write without the fused path).

tests/test_normals_loss_host.py checks this against an explicit mask formulation and against known answers.
"""
import math

import torch
import torch.nn.functional as F

EPS = 1e-12
DEFAULTS = dict(smoothing=2.0, min_depth=0.0, max_depth=math.inf, alpha_floor=1e-3)


def blur_weights(sigma, dtype=torch.float64, device="cpu"):
    """w_k ~ exp(-k^2 / 2 sigma^2), k = -2..2, normalised to 1 in float64 and rounded once to fp32 (sigma itself is the fp32
    value the library receives)."""
    s = float(torch.tensor(float(sigma), dtype=torch.float32))
    w = [math.exp(-(k * k) / (2.0 * s * s)) for k in range(-2, 3)]
    total = 0.0
    for x in w:
        total += x
    return torch.tensor([x / total for x in w], dtype=torch.float64).float().to(dtype=dtype, device=device)


def expected_depth(depth, alpha, alpha_floor):
    d = torch.where(torch.isfinite(depth), depth, torch.zeros_like(depth))       # (a non-finite depth is a hole either way)
    return d if alpha is None else d / alpha.clamp_min(alpha_floor)


def with_nans(x, lo, hi):
    """x where isfinite(x) & (x > lo) & (x < hi), NaN elsewhere."""
    valid = torch.isfinite(x) & (x > lo) & (x < hi)
    return torch.where(valid, x, torch.full_like(x, float("nan")))


def taps(x, dy, dx):
    """x [..., H, W] at the replicate-clamped coordinates (y + dy, x + dx)."""
    H, W = x.shape[-2:]
    yy = (torch.arange(H, device=x.device) + dy).clamp(0, H - 1)
    xx = (torch.arange(W, device=x.device) + dx).clamp(0, W - 1)
    return x.index_select(-2, yy).index_select(-1, xx)


def smooth(x, sigma):
    """The separable 5 x 5 blur (rows, then columns) of [B, H, W]; None: x itself."""
    if sigma is None:
        return x
    w = blur_weights(sigma, x.dtype, x.device)
    h = (((w[0] * taps(x, 0, -2) + w[1] * taps(x, 0, -1)) + w[2] * x) + w[3] * taps(x, 0, 1)) + w[4] * taps(x, 0, 2)
    return (((w[0] * taps(h, -2, 0) + w[1] * taps(h, -1, 0)) + w[2] * h) + w[3] * taps(h, 1, 0)) + w[4] * taps(h, 2, 0)


def rays(intr, H, W, dtype, device):
    """intr [B, 4] -> ((px - cx) / fx [B, 1, W], (py - cy) / fy [B, H, 1])."""
    fx, fy, cx, cy = (intr[:, k].view(-1, 1, 1) for k in range(4))
    px = torch.arange(W, dtype=dtype, device=device).view(1, 1, W)
    py = torch.arange(H, dtype=dtype, device=device).view(1, H, 1)
    return (px - cx) / fx, (py - cy) / fy


def sobel_vectors(S, intr):
    """S [B, H, W] finite -> (Gx, Gy) [B, 3, H, W]: Sobel / 8 of the camera-space points."""
    H, W = S.shape[1:]
    rx, ry = rays(intr, H, W, S.dtype, S.device)
    P = torch.stack([S * rx, S * ry, S], 1)
    t = lambda a, b: taps(P, a, b)
    Gx = 0.125 * (((t(-1, 1) - t(-1, -1)) + (t(1, 1) - t(1, -1))) + 2.0 * (t(0, 1) - t(0, -1)))
    Gy = 0.125 * (((t(1, -1) - t(-1, -1)) + (t(1, 1) - t(-1, 1))) + 2.0 * (t(1, 0) - t(-1, 0)))
    return Gx, Gy


def normals_of(S, intr):
    """S [B, H, W] with NaN = invalid -> (n [B, 3, H, W] finite everywhere, M [B, H, W]: all nine clamped taps valid)."""
    nine = sum(taps(S, a, b) for a in (-1, 0, 1) for b in (-1, 0, 1))
    M = torch.isfinite(nine)
    safe = torch.where(torch.isfinite(S), S, torch.ones_like(S))
    Gx, Gy = sobel_vectors(safe, intr)
    return F.normalize(torch.cross(Gx, Gy, dim=1), dim=1, eps=EPS), M


def _intr(intr, B, dtype, device):
    k = torch.as_tensor(intr).detach().to(device=device, dtype=dtype)
    return k.expand(B, 4) if k.dim() == 1 else k


def depth_normals(depth, intr, alpha=None, *, smoothing=2.0, alpha_floor=1e-3, min_depth=0.0, max_depth=math.inf):
    """[B, 3, H, W], NaN where invalid."""
    E = with_nans(expected_depth(depth, alpha, alpha_floor), max(min_depth, 0.0), max_depth)
    n, M = normals_of(smooth(E, smoothing), _intr(intr, depth.shape[0], depth.dtype, depth.device))
    return torch.where(M[:, None], n, torch.full_like(n, float("nan")))


def pixel_terms(depth, intr, *, gt_depth=None, gt_normals=None, alpha=None, smoothing=2.0, min_depth=0.0, max_depth=math.inf,
                alpha_floor=1e-3):
    """(0.5 (1 - n . t) [B, H, W] with 0 outside M, M [B, H, W])."""
    assert (gt_depth is None) != (gt_normals is None)
    k = _intr(intr, depth.shape[0], depth.dtype, depth.device)
    E = with_nans(expected_depth(depth, alpha, alpha_floor), 0.0, math.inf)
    n, M = normals_of(smooth(E, smoothing), k)
    if gt_depth is not None:
        t, Mt = normals_of(smooth(with_nans(gt_depth, min_depth, max_depth), smoothing), k)
    else:
        Mt = torch.isfinite(gt_normals).all(1)
        t = torch.where(Mt[:, None], gt_normals, torch.zeros_like(gt_normals))
    M = M & Mt
    dot = (n[:, 0] * t[:, 0] + n[:, 1] * t[:, 1]) + n[:, 2] * t[:, 2]
    term = 0.5 * (1.0 - dot)
    return torch.where(M, term, torch.zeros_like(term)), M


def terms(depth, intr, **kw):
    """(sum [B], cnt [B]) in the inputs' dtype."""
    term, M = pixel_terms(depth, intr, **kw)
    return term.flatten(1).sum(1), M.flatten(1).sum(1).to(depth.dtype)


def combine(total, cnt):
    """No valid pixel anywhere: exactly 0 (a plain mean of an empty set would give NaN)."""
    c = cnt.sum()
    return torch.where(c > 0, total.sum() / c.clamp_min(1.0), torch.zeros_like(c))


def normals_loss(depth, intr, **kw):
    return combine(*terms(depth, intr, **kw))


def _as(t, dtype, device):
    return None if t is None else torch.as_tensor(t).detach().to(device=device, dtype=dtype)


def _targets(kw, dtype, device):
    kw = dict(kw)
    for name in ("gt_depth", "gt_normals"):
        kw[name] = _as(kw.get(name), dtype, device)
    return kw


def _leaves(depth, alpha, dtype, device):
    d = _as(depth, dtype, device).requires_grad_(True)
    a = None if alpha is None else _as(alpha, dtype, device).requires_grad_(True)
    return d, a


def _grads(out, d, a):
    if out.grad_fn is None:
        return torch.zeros_like(d), (None if a is None else torch.zeros_like(a))
    got = torch.autograd.grad(out, [d] if a is None else [d, a], allow_unused=True)
    z = lambda t, like: torch.zeros_like(like) if t is None else t
    return z(got[0], d), (None if a is None else z(got[1], a))


def values(depth, intr, alpha=None, dtype=torch.float64, device="cpu", **kw):
    """(sum, cnt) in `dtype` on `device`, no graph."""
    with torch.no_grad():
        return terms(_as(depth, dtype, device), intr, alpha=_as(alpha, dtype, device), **_targets(kw, dtype, device))


def grad(depth, intr, alpha=None, g_sum=None, dtype=torch.float64, device="cpu", **kw):
    """autograd's d(sum_b g_sum[b] sum[b]) / d(depth, alpha) -> (g_depth, g_alpha | None)."""
    d, a = _leaves(depth, alpha, dtype, device)
    total, _ = terms(d, intr, alpha=a, **_targets(kw, dtype, device))
    return _grads((total * _as(g_sum, dtype, device)).sum(), d, a)


def loss_grad(depth, intr, alpha=None, dtype=torch.float64, device="cpu", **kw):
    """(loss, g_depth, g_alpha | None) through the scalar loss."""
    d, a = _leaves(depth, alpha, dtype, device)
    loss = normals_loss(d, intr, alpha=a, **_targets(kw, dtype, device))
    return (loss.detach(),) + _grads(loss, d, a)


def normals_values(depth, intr, alpha=None, dtype=torch.float64, device="cpu", **kw):
    with torch.no_grad():
        return depth_normals(_as(depth, dtype, device), intr, _as(alpha, dtype, device), **kw)


def normals_grad(depth, intr, alpha=None, g=None, dtype=torch.float64, device="cpu", **kw):
    """autograd's d(sum over the valid pixels of g . n) / d(depth, alpha) for a cotangent g [B, 3, H, W]."""
    d, a = _leaves(depth, alpha, dtype, device)
    n = depth_normals(d, intr, a, **kw)
    ok = torch.isfinite(n)
    return _grads((torch.where(ok, n, torch.zeros_like(n)) * _as(g, dtype, device)).sum(), d, a)
