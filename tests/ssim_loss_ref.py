"""Torch restatement of freesplat_amd/ssim_loss.py, written from the definitions (DESIGN.md "SSIM / photometric loss"),
differentiable by autograd: float64 on the CPU as the reference, or any dtype on any device as the eager yardstick (the
grouped separable conv2d form a user would write without the fused path).

Both conventions: 11-tap Gaussian (metrics_ref.gauss_weights), u = G*x, G*y, G*x^2, G*y^2, G*xy, v = n (u_xx - u_x^2) ...,
S = (2 u_x u_y + C1)(2 v_xy + C2) / ((u_x^2 + u_y^2 + C1)(v_x + v_y + C2)), x = ground truth, y = prediction.
  "skimage": 'valid' filter (no padding read), n = 121/120, mean over the [H-10, W-10] outputs, then channels.
  "3dgs":    zero padding by 5 (conv2d(padding=5)), n = 1, mean over the [H, W] outputs and channels.
closed_form_grad() is the gather the HIP backward implements, in the same dtype, without autograd.
"""
import torch
import torch.nn.functional as F

import metrics_ref as R

CONVENTIONS = ("skimage", "3dgs")


def _pad(convention):
    if convention not in CONVENTIONS:
        raise ValueError(convention)
    return R.RAD if convention == "3dgs" else 0


def _norm(convention):
    return 1.0 if convention == "3dgs" else R.COV_NORM


def _weights(like):
    return torch.from_numpy(R.gauss_weights()).to(device=like.device, dtype=like.dtype)


def gauss_filter(a, pad):
    """Separable Gaussian correlation of [B, C, H, W] as two grouped conv2d calls, zero padding `pad` in both axes."""
    C = a.shape[1]
    w = _weights(a)
    a = F.conv2d(a, w.view(1, 1, -1, 1).expand(C, 1, -1, 1), padding=(pad, 0), groups=C)
    return F.conv2d(a, w.view(1, 1, 1, -1).expand(C, 1, 1, -1), padding=(0, pad), groups=C)


def _terms(pred, gt, convention):
    pad, n = _pad(convention), _norm(convention)
    x, y = gt, pred
    ux, uy = gauss_filter(x, pad), gauss_filter(y, pad)
    uxx, uyy, uxy = gauss_filter(x * x, pad), gauss_filter(y * y, pad), gauss_filter(x * y, pad)
    vx, vy, vxy = n * (uxx - ux * ux), n * (uyy - uy * uy), n * (uxy - ux * uy)
    a1, a2 = 2 * ux * uy + R.C1, 2 * vxy + R.C2
    b1, b2 = ux * ux + uy * uy + R.C1, vx + vy + R.C2
    return ux, uy, a1, a2, b1, b2


def ssim_map(pred, gt, convention):
    """S per averaged output: [B, C, H-10, W-10] ("skimage") or [B, C, H, W] ("3dgs"), in the inputs' dtype."""
    _, _, a1, a2, b1, b2 = _terms(pred, gt, convention)
    return (a1 * a2) / (b1 * b2)


def ssim(pred, gt, convention):
    return ssim_map(pred, gt, convention).mean(dim=(1, 2, 3))


def l1_mean(pred, gt):
    return (pred - gt).abs().mean(dim=(1, 2, 3))


def photometric_loss(pred, gt, lambda_dssim=0.2, convention="3dgs"):
    return (1.0 - lambda_dssim) * l1_mean(pred, gt).mean() + lambda_dssim * (1.0 - ssim(pred, gt, convention).mean())


def _as(t, dtype, device):
    return torch.as_tensor(t).detach().to(device=device, dtype=dtype)


def values(pred, gt, convention, dtype=torch.float64, device="cpu"):
    """(ssim [B], l1_mean [B]) in `dtype` on `device`."""
    p, g = _as(pred, dtype, device), _as(gt, dtype, device)
    return ssim(p, g, convention), l1_mean(p, g)


def grad(pred, gt, convention, g_ssim=None, g_l1=None, dtype=torch.float64, device="cpu"):
    """autograd's d(sum_b g_ssim[b] ssim[b] + g_l1[b] l1_mean[b]) / d pred; a None cotangent leaves that term out."""
    p, g = _as(pred, dtype, device).requires_grad_(True), _as(gt, dtype, device)
    total = 0
    if g_ssim is not None:
        total = total + (ssim(p, g, convention) * _as(g_ssim, dtype, device)).sum()
    if g_l1 is not None:
        total = total + (l1_mean(p, g) * _as(g_l1, dtype, device)).sum()
    return torch.autograd.grad(total, p)[0]


def photometric_grad(pred, gt, lambda_dssim, convention, dtype=torch.float64, device="cpu"):
    p, g = _as(pred, dtype, device).requires_grad_(True), _as(gt, dtype, device)
    loss = photometric_loss(p, g, lambda_dssim, convention)
    return loss.detach(), torch.autograd.grad(loss, p)[0]


def closed_form_grad(pred, gt, convention, g_ssim=None, g_l1=None, dtype=torch.float64):
    """The backward as a gather, no autograd: with P_yy = -n S / b2, P_xy = 2 n a1 / (b1 b2),
    P_y = 2 u_x a2 / (b1 b2) - 2 u_y S / b1 - 2 u_y P_yy - u_x P_xy over the averaged outputs,
        dL/dpred = G*(g P_y) + 2 pred G*(g P_yy) + gt G*(g P_xy) + g_l1 / (C H W) sign(pred - gt),
    g = g_ssim / (averaged outputs of a view), G* over the maps zero-extended by 10 ("skimage") or by 5 ("3dgs")."""
    p, x = _as(pred, dtype, "cpu"), _as(gt, dtype, "cpu")
    B, C, H, W = p.shape
    out = torch.zeros_like(p)
    if g_ssim is not None:
        n = _norm(convention)
        ux, uy, a1, a2, b1, b2 = _terms(p, x, convention)
        S = (a1 * a2) / (b1 * b2)
        g = (_as(g_ssim, dtype, "cpu") / (C * S.shape[2] * S.shape[3])).view(B, 1, 1, 1)
        P_yy = -n * S / b2
        P_xy = 2 * n * a1 / (b1 * b2)
        P_y = 2 * ux * a2 / (b1 * b2) - 2 * uy * S / b1 - 2 * uy * P_yy - ux * P_xy
        back = 2 * R.RAD - _pad(convention)          # zero extension that brings the maps back to [H, W]
        out = gauss_filter(g * P_y, back) + 2 * p * gauss_filter(g * P_yy, back) + x * gauss_filter(g * P_xy, back)
    if g_l1 is not None:
        out = out + (_as(g_l1, dtype, "cpu") / (C * H * W)).view(B, 1, 1, 1) * torch.sign(p - x)
    return out
