"""Differentiable SSIM and the `(1 - lambda) L1 + lambda (1 - SSIM)` photometric loss on the device, through
fs_ssim_loss_forward / fs_ssim_loss_backward (libfreesplat_hip.so, include/freesplat_amd_loss.h, csrc/ssim_loss.hip).

Two conventions (DESIGN.md "SSIM / photometric loss"):
  "skimage"  the SSIM `metrics.compute_ssim` reports: sample covariance (121/120), mean over the interior [5, H-5) x [5, W-5),
             no padding value read, images of at least 11 x 11;
  "3dgs"     the usual training form: the image zero-padded by 5 as conv2d(padding=5) does, population covariance, mean over
             all H x W outputs, any image size.
Both: 11-tap Gaussian (sigma 1.5), C1 = 1e-4, C2 = 9e-4, data range 1, no clipping.

One forward library call gives the per-view SSIM and the per-view mean |predicted - ground_truth|; one backward call gives the
gradient of both with respect to `predicted`, deterministically (a gather, no atomics).  `ground_truth` gets no gradient.
For the backward the forward keeps three floats per averaged output (`saved_bytes`); without a pending backward nothing is
kept.  Device tensors only: there is no CPU / eager path.
"""
from __future__ import annotations

import torch
from torch import Tensor

from . import _args, _lib

WIN = 11                 # window of both conventions; the smallest image "skimage" accepts
TILE_W, TILE_H = 246, 64  # pixels of a plane one workgroup owns (csrc/ssim_loss.hip kTileW, kTileH); tests place shapes by it
CONVENTIONS = {"skimage": _lib.SSIM_SKIMAGE, "3dgs": _lib.SSIM_3DGS}


def _flags(convention: str) -> int:
    if convention not in CONVENTIONS:
        raise ValueError(f"freesplat_amd.ssim_loss: convention must be one of {sorted(CONVENTIONS)}, got {convention!r}")
    return CONVENTIONS[convention]


def _images(predicted: Tensor, ground_truth: Tensor, convention: str):
    flags = _flags(convention)
    if isinstance(ground_truth, Tensor) and ground_truth.requires_grad and torch.is_grad_enabled():
        raise RuntimeError("freesplat_amd.ssim_loss: ground_truth gets no gradient from the fused loss; detach it (only "
                           "`predicted` is differentiated)")
    pred = _args.device_f32(predicted, "predicted", "freesplat_amd.ssim_loss")
    gt = _args.device_f32(ground_truth, "ground_truth", "freesplat_amd.ssim_loss").detach()
    if pred.dim() != 4 or pred.shape != gt.shape:
        raise ValueError(f"freesplat_amd.ssim_loss: expected two [B, C, H, W] tensors of one shape, got "
                         f"{tuple(pred.shape)} and {tuple(gt.shape)}")
    if pred.device != gt.device:
        raise ValueError(f"freesplat_amd.ssim_loss: tensors on {pred.device} and {gt.device}")
    B, C, H, W = pred.shape
    if B == 0 or C == 0 or H == 0 or W == 0:
        raise ValueError("freesplat_amd.ssim_loss: empty batch")
    if convention == "skimage" and (H < WIN or W < WIN):
        raise ValueError(f"freesplat_amd.ssim_loss: win_size exceeds image extent ({H}x{W} < {WIN}x{WIN}); the '3dgs' "
                         "convention pads and takes any size")
    return pred, gt, flags


def saved_bytes(B: int, C: int, H: int, W: int, convention: str) -> int:
    """Bytes the forward keeps for a pending backward (three fp32 maps over the averaged outputs)."""
    return int(_lib.lib().fs_ssim_loss_saved_bytes(B, C, H, W, _flags(convention)))


class _SsimL1(torch.autograd.Function):
    """pred, gt [B, C, H, W] -> (ssim [B], l1_mean [B]) float32.  `saved` is allocated by the caller (None: no backward is
    pending): torch.is_grad_enabled() is always False inside forward, so the decision cannot be taken here."""

    @staticmethod
    def forward(ctx, pred, gt, saved, flags):
        B, C, H, W = pred.shape
        L = _lib.lib()
        dev = pred.device
        scratch = torch.empty(L.fs_ssim_loss_scratch_bytes(B, C, H, W, flags), dtype=torch.uint8, device=dev)
        out = torch.empty(2, B, dtype=torch.float64, device=dev)
        p = _lib.ptr
        _lib.launch("fs_ssim_loss_forward", B, C, H, W, flags, p(pred), p(gt), p(out[0]), p(out[1]), p(saved), p(scratch))
        ctx.flags = flags
        ctx.set_materialize_grads(False)
        if saved is not None:
            ctx.save_for_backward(pred, gt, saved)
        return out[0].float(), out[1].float()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_ssim, g_l1):
        if g_ssim is None and g_l1 is None:
            return None, None, None, None
        pred, gt, saved = ctx.saved_tensors
        B, C, H, W = pred.shape
        g_ssim = None if g_ssim is None else g_ssim.float().contiguous()
        g_l1 = None if g_l1 is None else g_l1.float().contiguous()
        g_pred = torch.empty(B, C, H, W, device=pred.device)
        p = _lib.ptr
        _lib.launch("fs_ssim_loss_backward", B, C, H, W, ctx.flags, p(pred), p(gt), p(g_ssim), p(g_l1), p(saved), p(g_pred), None)
        return g_pred, None, None, None


def ssim_and_l1(predicted: Tensor, ground_truth: Tensor, convention: str = "skimage"):
    """(ssim [B], l1_mean [B]) float32 from one library call, both differentiable with respect to `predicted`:
    l1_mean = mean over c, h, w of |predicted - ground_truth|."""
    pred, gt, flags = _images(predicted, ground_truth, convention)
    saved = None
    if torch.is_grad_enabled() and pred.requires_grad:
        B, C, H, W = pred.shape
        saved = torch.empty(_lib.lib().fs_ssim_loss_saved_bytes(B, C, H, W, flags) // 4, device=pred.device)
    return _SsimL1.apply(pred, gt, saved, flags)


def ssim(predicted: Tensor, ground_truth: Tensor, convention: str = "skimage") -> Tensor:
    """[B] float32 SSIM of each view, differentiable with respect to `predicted`."""
    return ssim_and_l1(predicted, ground_truth, convention)[0]


def dssim_loss(predicted: Tensor, ground_truth: Tensor, convention: str = "skimage") -> Tensor:
    """The scalar 1 - mean over the views of ssim."""
    return 1.0 - ssim(predicted, ground_truth, convention).mean()


def photometric_loss(predicted: Tensor, ground_truth: Tensor, lambda_dssim: float = 0.2, convention: str = "3dgs") -> Tensor:
    """The scalar (1 - lambda) mean |predicted - ground_truth| + lambda (1 - mean ssim): one forward and one backward library
    call for both terms (the per-view means are combined by a few torch operations on [B] tensors)."""
    s, l1 = ssim_and_l1(predicted, ground_truth, convention)
    return (1.0 - lambda_dssim) * l1.mean() + lambda_dssim * (1.0 - s.mean())
