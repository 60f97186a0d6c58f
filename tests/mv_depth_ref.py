"""Torch restatement of freesplat_amd/mv_depth_loss.py, written from the definitions (DESIGN.md "Multi-view depth loss") with
explicit indexing (no grid_sample).  Dtype- and device-generic and differentiable by autograd: float64 on the CPU as the
reference, or float32 on a chosen device as the eager yardstick (what a user would write without the fused path: per source a
projection chain over [B, 3, H, W], a gather, the masks and a masked sum).

A quantity that a mask discards is replaced by 1 under torch.where before a logarithm or a division, so that autograd never
multiplies a zero cotangent with a NaN.

tests/test_mv_depth_loss_host.py checks this against the reference's MVDepthLoss and ScaleInvariantLoss (tests/golden/
mv_depth_small.npz) and against finite differences.
"""
import math

import torch

EPS = 1e-8


def f32(x):
    """A scalar as the library receives it: rounded to fp32 (alpha_floor = 1e-3 is not a float; an alpha stored as
    float32(1e-3) EQUALS the floor the kernels see and is larger than the double 1e-3)."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def expected_depth(depth, alpha, alpha_floor):
    """(E with a non-finite depth replaced by 1, ok: E is finite).  max(alpha, floor) is written with torch.where, whose
    gradient is the definition's: dE / dalpha = -depth / alpha^2 where alpha > alpha_floor, else 0 (clamp_min would pass the
    gradient at alpha == alpha_floor)."""
    fin = torch.isfinite(depth)
    d = torch.where(fin, depth, torch.ones_like(depth))
    E = d if alpha is None else d / torch.where(alpha > alpha_floor, alpha, torch.full_like(alpha, alpha_floor))
    return E, fin & torch.isfinite(E)


def valid(x, lo, hi):
    return torch.isfinite(x) & (x > lo) & (x < hi)


def pair_transforms(intr, cam_to_world, src_intr, src_world_to_cam, src_index=None, dtype=torch.float64):
    """[B, K, 3, 4] = [A | t] in `dtype`: M = K_s T_s<-w T_w<-c, A = M[:, :3] K_c^-1, t = M[:, 3].  intr [4] | [B, 4]; sources
    [B, K, ...], or a pool [S, ...] with src_index [B, K] (an index out of range gives zeros)."""
    c2w = torch.as_tensor(cam_to_world).to(dtype)
    B = c2w.shape[0]
    w2s = torch.as_tensor(src_world_to_cam).to(dtype)
    ks = torch.as_tensor(src_intr).to(dtype)
    kc = torch.as_tensor(intr).to(dtype)
    kc = kc.expand(B, 4) if kc.dim() == 1 else kc
    if src_index is not None:
        S = w2s.shape[0]
        ks = ks.expand(S, 4) if ks.dim() == 1 else ks
    K = w2s.shape[1] if src_index is None else src_index.shape[1]
    out = torch.zeros(B, K, 3, 4, dtype=dtype)
    for b in range(B):
        Kc_inv = torch.linalg.inv(torch.tensor([[kc[b, 0], 0.0, kc[b, 2]], [0.0, kc[b, 1], kc[b, 3]], [0.0, 0.0, 1.0]], dtype=dtype))
        for k in range(K):
            if src_index is None:
                T, q = w2s[b, k], (ks if ks.dim() == 1 else ks[b, k])
            else:
                i = int(src_index[b, k])
                if not 0 <= i < S:
                    continue
                T, q = w2s[i], ks[i]
            Ks = torch.tensor([[q[0], 0.0, q[2]], [0.0, q[1], q[3]], [0.0, 0.0, 1.0]], dtype=dtype)
            M = Ks @ (T @ c2w[b])[:3]
            out[b, k] = torch.cat([M[:, :3] @ Kc_inv, M[:, 3:]], 1)
    return out


def _sources(src, src_index, B, K):
    """-> (maps [B, K, Hs, Ws], on [B, K]: the pair has a source)."""
    if src_index is None:
        return src, torch.ones(B, K, dtype=torch.bool, device=src.device)
    idx = src_index.to(src.device).long()
    on = (idx >= 0) & (idx < src.shape[0])
    return src[idx.clamp(0, src.shape[0] - 1)], on


def pixel_terms(depth, gt, src, pairs, alpha=None, *, src_index=None, occlusion=1.05, min_depth=0.0, max_depth=math.inf,
                alpha_floor=1e-3):
    """(r [B, K, H, W] with 0 where not selected, selected [B, K, H, W])."""
    occlusion, min_depth, max_depth, alpha_floor = f32(occlusion), f32(min_depth), f32(max_depth), f32(alpha_floor)
    B, H, W = depth.shape
    K = pairs.shape[1]
    dt, dev = depth.dtype, depth.device
    maps, on = _sources(src, src_index, B, K)
    Hs, Ws = maps.shape[-2:]
    E, E_ok = expected_depth(depth, alpha, alpha_floor)
    V0 = valid(gt, min_depth, max_depth)
    x = torch.arange(W, dtype=dt, device=dev).view(1, 1, W).expand(B, H, W)
    y = torch.arange(H, dtype=dt, device=dev).view(1, H, 1).expand(B, H, W)
    pix = torch.stack([x, y, torch.ones_like(x)], 1)                                   # [B, 3, H, W]
    g = torch.where(V0, gt, torch.ones_like(gt))
    rs, sel = [], []
    for k in range(K):
        A, t = pairs[:, k, :, :3], pairs[:, k, :, 3]
        ray = torch.einsum("bij,bjhw->bihw", A, pix)
        q = g[:, None] * ray + t[:, :, None, None]
        z = q[:, 2]
        zq = z + EPS
        persp = z.abs() > EPS
        den = torch.where(persp, zq, torch.ones_like(zq))
        ix, iy = torch.round(q[:, 0] / den), torch.round(q[:, 1] / den)                # half to even
        inside = (ix >= 0) & (ix < Ws) & (iy >= 0) & (iy < Hs)
        flat = (torch.where(inside, iy, torch.zeros_like(iy)) * Ws + torch.where(inside, ix, torch.zeros_like(ix))).long()
        S = torch.gather(maps[:, k].reshape(B, Hs * Ws), 1, flat.view(B, H * W)).view(B, H, W)
        S = torch.where(inside, S, torch.zeros_like(S))
        visible = V0 & valid(S, min_depth, max_depth) & (zq > 0) & (zq < occlusion * S) & on[:, k].view(B, 1, 1)
        zp = E * ray[:, 2] + t[:, 2, None, None] + EPS
        selected = visible & E_ok & torch.isfinite(zp) & (zp > 0)
        one = torch.ones_like(zp)
        r = torch.log(torch.where(selected, zp, one)) - torch.log(torch.where(selected, S, one))
        rs.append(torch.where(selected, r, torch.zeros_like(r)))
        sel.append(selected)
    return torch.stack(rs, 1), torch.stack(sel, 1)


def terms(depth, gt, src, pairs, alpha=None, **kw):
    """(sum [B, K], cnt [B, K]) in the inputs' dtype."""
    r, sel = pixel_terms(depth, gt, src, pairs, alpha, **kw)
    return r.abs().flatten(2).sum(2), sel.flatten(2).sum(2).to(depth.dtype)


def combine(total, cnt):
    return (total.sum(0) / cnt.sum(0).clamp_min(1.0)).mean()


def mv_depth_loss(depth, gt, src, pairs, alpha=None, **kw):
    return combine(*terms(depth, gt, src, pairs, alpha, **kw))


def residuals(depth, gt, src, pairs, alpha=None, **kw):
    """[B, K, H, W], NaN where not selected."""
    r, sel = pixel_terms(depth, gt, src, pairs, alpha, **kw)
    return torch.where(sel, r, torch.full_like(r, float("nan")))


def si_terms(depth, gt, alpha=None, *, min_depth=0.0, max_depth=math.inf, alpha_floor=1e-3):
    """(s1 [B], s2 [B], n [B]) in the inputs' dtype."""
    min_depth, max_depth, alpha_floor = f32(min_depth), f32(max_depth), f32(alpha_floor)
    E, E_ok = expected_depth(depth, alpha, alpha_floor)
    P = valid(gt, min_depth, max_depth) & E_ok & (E > 0)
    one = torch.ones_like(E)
    d = torch.log(torch.where(P, gt, one)) - torch.log(torch.where(P, E, one))
    d = torch.where(P, d, torch.zeros_like(d))
    return d.flatten(1).sum(1), (d * d).flatten(1).sum(1), P.flatten(1).sum(1).to(depth.dtype)


def combine_si(s1, s2, n, si_lambda=0.85):
    N = n.sum().clamp_min(1.0)
    mean = s1.sum() / N
    var = s2.sum() / N - si_lambda * mean * mean
    pos = var > 0
    return torch.where(pos, torch.where(pos, var, torch.ones_like(var)).sqrt(), torch.zeros_like(var))


def scale_invariant_loss(depth, gt, alpha=None, si_lambda=0.85, **kw):
    return combine_si(*si_terms(depth, gt, alpha, **kw), si_lambda)


# ---- evaluation in a chosen dtype on a chosen device -------------------------------------------------------------------------

def _as(t, dtype, device):
    if t is None:
        return None
    t = torch.as_tensor(t).detach()
    return t.to(device) if not t.is_floating_point() else t.to(device=device, dtype=dtype)


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


def _mv_args(c, dtype, device):
    kw = dict(c.get("kw", {}))
    kw["src_index"] = _as(c.get("src_index"), dtype, device)
    return (_as(c["gt"], dtype, device), _as(c["src"], dtype, device), _as(c["pairs"], dtype, device)), kw


def mv_values(c, dtype=torch.float64, device="cpu"):
    """(sum, cnt, residuals) of a case dict (tests/mv_depth_cases.py), no graph."""
    args, kw = _mv_args(c, dtype, device)
    with torch.no_grad():
        d, a = _as(c["depth"], dtype, device), _as(c["alpha"], dtype, device)
        return terms(d, *args, a, **kw) + (residuals(d, *args, a, **kw),)


def mv_grad(c, g_sum, dtype=torch.float64, device="cpu"):
    """autograd's d(sum_bk g_sum[b,k] sum[b,k]) / d(depth, alpha) -> (g_depth, g_alpha | None)."""
    args, kw = _mv_args(c, dtype, device)
    d, a = _leaves(c["depth"], c["alpha"], dtype, device)
    total, _ = terms(d, *args, a, **kw)
    return _grads((total * _as(g_sum, dtype, device)).sum(), d, a)


def mv_loss_grad(c, dtype=torch.float64, device="cpu"):
    """(loss, g_depth, g_alpha | None) through the scalar loss."""
    args, kw = _mv_args(c, dtype, device)
    d, a = _leaves(c["depth"], c["alpha"], dtype, device)
    loss = mv_depth_loss(d, *args, a, **kw)
    return (loss.detach(),) + _grads(loss, d, a)


def _si_kw(c):
    return {k: v for k, v in c.get("kw", {}).items() if k != "occlusion"}


def si_values(c, dtype=torch.float64, device="cpu"):
    with torch.no_grad():
        return si_terms(_as(c["depth"], dtype, device), _as(c["gt"], dtype, device), _as(c["alpha"], dtype, device), **_si_kw(c))


def si_grad(c, g1, g2, dtype=torch.float64, device="cpu"):
    d, a = _leaves(c["depth"], c["alpha"], dtype, device)
    s1, s2, _ = si_terms(d, _as(c["gt"], dtype, device), a, **_si_kw(c))
    return _grads((s1 * _as(g1, dtype, device)).sum() + (s2 * _as(g2, dtype, device)).sum(), d, a)


def si_loss_grad(c, dtype=torch.float64, device="cpu", si_lambda=0.85):
    d, a = _leaves(c["depth"], c["alpha"], dtype, device)
    loss = scale_invariant_loss(d, _as(c["gt"], dtype, device), a, si_lambda, **_si_kw(c))
    return (loss.detach(),) + _grads(loss, d, a)
