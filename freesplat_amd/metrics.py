"""Evaluation metrics on the device: SSIM / PSNR (src/evaluation/metrics.py:11-19, 37-52) and the depth metrics of
src/model/model_wrapper.py:90-110, through fs_image_metrics / fs_depth_metrics (libfreesplat_hip.so).

The reference's compute_ssim copies every view to the host and runs skimage on it one view at a time; here one call
computes SSIM and the MSE of compute_psnr for a whole batch, and the depth metrics' ~15 torch ops are one pass.  Nothing
here reads a value back to the host: results stay on the device until the caller asks for them.
SSIM is skimage's structural_similarity(gt, pred, win_size=11, gaussian_weights=True, channel_axis=0, data_range=1.0)
(DESIGN.md "Evaluation metrics": weights, covariance normalisation, crop, precision).
"""
from __future__ import annotations

import torch
from torch import Tensor

from . import _args, _lib

WIN = 11                # skimage raises "win_size exceeds image extent" below this
DEPTH_THRESHOLD = 0.5   # model_wrapper.py:95 `gt_bN > 0.5`


def _device_f32(t: Tensor, what: str) -> Tensor:
    return _args.device_f32(t, what, "freesplat_amd.metrics").detach()


def _images(ground_truth: Tensor, predicted: Tensor):
    gt = _device_f32(ground_truth, "ground_truth")
    pred = _device_f32(predicted, "predicted")
    if gt.dim() != 4 or gt.shape != pred.shape:
        raise ValueError(f"freesplat_amd.metrics: expected two [B, C, H, W] tensors of one shape, got "
                         f"{tuple(gt.shape)} and {tuple(pred.shape)}")
    if gt.device != pred.device:
        raise ValueError(f"freesplat_amd.metrics: tensors on {gt.device} and {pred.device}")
    B, C, H, W = gt.shape
    if H < WIN or W < WIN:
        raise ValueError(f"freesplat_amd.metrics: win_size exceeds image extent ({H}x{W} < {WIN}x{WIN})")
    if B == 0 or C == 0:
        raise ValueError("freesplat_amd.metrics: empty batch")
    return gt, pred


@torch.no_grad()
def _image_metrics(gt: Tensor, pred: Tensor, return_map: bool):
    """-> (ssim [B] float64, mse [B] float64, map [B, C, H-10, W-10] | None) from ONE fs_image_metrics call."""
    B, C, H, W = gt.shape
    L = _lib.lib()
    dev = gt.device
    scratch = torch.empty(L.fs_image_metrics_scratch_bytes(B, C, H, W), dtype=torch.uint8, device=dev)
    ssim = torch.empty(B, dtype=torch.float64, device=dev)
    mse = torch.empty(B, dtype=torch.float64, device=dev)
    smap = torch.empty(B, C, H - WIN + 1, W - WIN + 1, device=dev) if return_map else None
    p = _lib.ptr
    _lib.launch("fs_image_metrics", B, C, H, W, p(gt), p(pred), p(ssim), p(mse), p(smap), p(scratch))
    return ssim, mse, smap


def _psnr(mse: Tensor) -> Tensor:
    return -10 * mse.float().log10()            # fp32 as the reference's; mse == 0 gives inf


@torch.no_grad()
def compute_psnr(ground_truth: Tensor, predicted: Tensor) -> Tensor:
    """[batch] PSNR of the clipped images (metrics.py:11-19), float32 on the inputs' device."""
    gt, pred = _images(ground_truth, predicted)
    return _psnr(_image_metrics(gt, pred, False)[1])


@torch.no_grad()
def compute_ssim(ground_truth: Tensor, predicted: Tensor) -> Tensor:
    """[batch] SSIM (metrics.py:37-52) on predicted.device in predicted.dtype.  Not clipped (the reference does not
    clip either; compute_metrics clips `rgb` before the call)."""
    gt, pred = _images(ground_truth, predicted)
    return _image_metrics(gt, pred, False)[0].to(predicted.dtype)


@torch.no_grad()
def image_metrics(gt: Tensor, pred: Tensor, return_map: bool = False):
    """(psnr [B] float32, ssim [B] float64[, ssim_map [B, C, H-10, W-10] float32]) from one kernel call."""
    gt, pred = _images(gt, pred)
    ssim, mse, smap = _image_metrics(gt, pred, return_map)
    return (_psnr(mse), ssim, smap) if return_map else (_psnr(mse), ssim)


@torch.no_grad()
def depth_metrics(gt: Tensor, pred: Tensor) -> dict:
    """gt, pred [..., H, W] (leading dims = views) -> per-view float64 tensors abs_diff, abs_rel, delta_25, delta_10 with
    depth_render_metrics' rules: valid pixels gt > 0.5; abs_* are nanmeans (NaN terms dropped); a NaN ratio counts as
    outside delta; a view without valid pixels gives NaN."""
    g = _device_f32(gt, "gt")
    p = _device_f32(pred, "pred")
    if g.shape != p.shape or g.dim() < 2:
        raise ValueError(f"freesplat_amd.metrics: depth shapes {tuple(g.shape)} and {tuple(p.shape)}")
    HW = g.shape[-1] * g.shape[-2]
    n = g.numel() // HW if HW else 0
    if n == 0 or HW == 0:
        raise ValueError("freesplat_amd.metrics: empty depth maps")
    L = _lib.lib()
    scratch = torch.empty(L.fs_depth_metrics_scratch_bytes(n, HW), dtype=torch.uint8, device=g.device)
    out = torch.empty(6, n, dtype=torch.float64, device=g.device)
    _lib.launch("fs_depth_metrics", n, HW, _lib.ptr(g), _lib.ptr(p), DEPTH_THRESHOLD, _lib.ptr(out), _lib.ptr(scratch))
    n_valid, n_nonnan, s_abs, s_rel, n25, n10 = out
    return {"abs_diff": s_abs / n_nonnan, "abs_rel": s_rel / n_nonnan, "delta_25": n25 / n_valid, "delta_10": n10 / n_valid}


@torch.no_grad()
def depth_render_metrics(prediction, batch):
    """Drop-in for model_wrapper.depth_render_metrics: (abs_diff, abs_rel, delta_25, delta_10) as 0-d float32 tensors,
    each the mean over the b*v views of the per-view value (NaN of a view without valid pixels propagates)."""
    if "depth" not in batch["target"]:
        return torch.tensor(0.0), torch.tensor(0.0), torch.tensor(0.0), torch.tensor(0.0)
    target = batch["target"]["depth"].squeeze(2)
    m = depth_metrics(target, prediction.depth)
    return tuple(m[k].mean().float() for k in ("abs_diff", "abs_rel", "delta_25", "delta_10"))
