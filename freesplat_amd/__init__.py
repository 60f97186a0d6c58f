"""freesplat_amd -- MI355X-native (gfx950) implementation of FreeSplat's data-parallel hot path.

Only what the path needs lives here: `csrc/` (hand-written HIP kernels + the C ABI declared in
include/freesplat_amd.h), and the host-side mirrors of the reference's operator interfaces:

  rasterizer.py   GaussianRasterizationSettings / GaussianRasterizer  (diff_gaussian_rasterization_depth)
  decoder.py      frame_views / render_cuda / render_views / DecoderSplattingCUDA (src/model/decoder/)
  metrics.py      compute_ssim / compute_psnr / depth_render_metrics on the device (src/evaluation/metrics.py)
  ssim_loss.py    differentiable SSIM and the (1 - lambda) L1 + lambda (1 - SSIM) photometric loss (no reference counterpart)
  normals_loss.py depth -> surface normals and the cosine normals loss (src/loss/losses.py NormalsLoss, restated)
  mv_depth_loss.py multi-view depth consistency and scale-invariant depth losses (src/loss/losses.py MVDepthLoss and
                  ScaleInvariantLoss, restated)
  exposure.py     per-view affine exposure compensation: apply_exposure, fit_exposure, color_corrected, Exposure (no reference
                  counterpart; exported here)
  transform.py    similarity transforms of Gaussian scenes: transform_gaussians, rotate_sh, sh_rotation_matrices,
                  transform_cameras, similarity_inverse, compose (the reference's src/misc/sh_rotation.py rotate_sh, restated
                  in the rasterizer's own basis; exported here)
  compat/         importable `diff_gaussian_rasterization_depth` module for an unmodified reference tree

There is no CPU or eager fallback: the ops raise if libfreesplat_hip.so is missing.
"""
__version__ = "0.1.0"

_EXPOSURE = ("apply_exposure", "fit_exposure", "color_corrected", "Exposure")
_TRANSFORM = ("transform_gaussians", "rotate_sh", "sh_rotation_matrices", "transform_cameras", "similarity_inverse", "compose",
              "similarity_matrix")


def __getattr__(name):
    # resolved on first use: importing the package itself stays free of torch
    if name in _EXPOSURE:
        from . import exposure
        return getattr(exposure, name)
    if name in _TRANSFORM:
        from . import transform
        return getattr(transform, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
