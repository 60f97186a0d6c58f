/*
 * freesplat_amd_loss.h -- training-loss entry points of libfreesplat_hip.so (MI355X / gfx950), beside freesplat_amd.h.
 *
 * Same rules as the main header: plain device pointers + sizes + a hipStream_t (passed as void*), an int status
 * (FS_OK, FS_ERR_*), NO allocation, NO host synchronisation, stream-ordered and hipGraph-capturable, arguments validated
 * before anything touches a device, fs_last_error() text after a failed launch.  Dense row-major fp32 unless noted.
 *
 * The declarations live in a header of their own with a revision of their own (FS_LOSS_API_VERSION): FS_ABI_VERSION and
 * the symbol set of freesplat_amd.h do not change.  A binding checks fs_loss_api_version() next to fs_abi_version().
 */
#ifndef FREESPLAT_AMD_LOSS_H
#define FREESPLAT_AMD_LOSS_H

#include "freesplat_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS_LOSS_API_VERSION 1
int fs_loss_api_version(void);

/* ------------------------------------------------------------------------------------ *
 * SSIM + L1 photometric loss, forward and backward                                      *
 * ------------------------------------------------------------------------------------ */

/* `flags` is exactly one of the two conventions.  Both: separable 11-tap Gaussian, sigma 1.5, weights normalised in double
 * and used in fp32; C1 = 1e-4, C2 = 9e-4; u = G*x, G*y, G*x^2, G*y^2, G*xy, v_x = n (u_xx - u_x^2), v_y, v_xy alike,
 *   S = (2 u_x u_y + C1)(2 v_xy + C2) / ((u_x^2 + u_y^2 + C1)(v_x + v_y + C2)).
 * FS_SSIM_SKIMAGE: the SSIM of fs_image_metrics (skimage.metrics.structural_similarity, win_size=11, gaussian_weights=True,
 *   data_range=1): n = 121/120, S averaged over the interior [5,H-5) x [5,W-5) of every channel, then over channels; no
 *   padding value is ever read; H, W >= 11.
 * FS_SSIM_3DGS: the image zero-padded by 5 as conv2d(padding=5) does, n = 1, S averaged over all H*W outputs and the
 *   channels; any H, W >= 1. */
#define FS_SSIM_SKIMAGE 1
#define FS_SSIM_3DGS 2

/* pred, gt [B,C,H,W] -> per view ssim[B] and l1_mean[B] = mean over c, h, w of |pred - gt| (no clipping), both double.
 * Per-pixel arithmetic fp32, sums fp64 in a fixed order, no atomics: a view's values are the same bits whatever the batch,
 * the stream or the run.  Identical images give ssim exactly 1.
 *   saved: NULL (no backward will follow), or fs_ssim_loss_saved_bytes(B, C, H, W, flags) bytes that receive three fp32 maps
 *     per (view, channel) plane over the averaged outputs ([H-10, W-10] resp. [H, W]): the partial derivatives of S with
 *     respect to G*y^2, G*xy and G*y (y = pred), the last one re-centred about 0.5 (see fs_ssim_loss_backward).  Opaque
 *     to the caller; 12 bytes per output.
 *   scratch: fs_ssim_loss_scratch_bytes(B, C, H, W, flags) bytes, free for reuse once the call's work has run.
 * fs_ssim_loss_backward writes g_pred [B,C,H,W] in full (it does not rely on a zeroed buffer), a gather without atomics:
 *   g_pred(q) = g_ssim[b] / n_out * ( G*(P_y')(q) + 2 (pred(q) - 0.5) G*(P_yy)(q) + (gt(q) - 0.5) G*(P_xy)(q) )
 *             + g_l1[b] / (C H W) * sign(pred(q) - gt(q)),                                   sign(0) = 0,
 *   with G* the same filter over the saved maps zero-extended (by 10 for FS_SSIM_SKIMAGE: border pixels of pred receive
 *   gradient from the interior windows that cover them; a `same` zero-padded pass for FS_SSIM_3DGS), n_out the number of
 *   averaged outputs of a view, and P_y' = P_y + P_yy + P_xy / 2 (the identity that moves the 0.5 out of the products).
 *   g_ssim[B], g_l1[B]: per-view cotangents in device memory (read by the kernel, no host sync); either may be NULL (that
 *   term is left out; `saved` is then not read for a NULL g_ssim), not both.  pred, gt, flags and the sizes must be those
 *   of the forward call that filled `saved`.  scratch is reserved: not read or written in this revision, may be NULL.
 * Sizes <= 0, a NULL required pointer, a `flags` value other than the two above, or H or W < 11 under FS_SSIM_SKIMAGE:
 * FS_ERR_INVALID_ARG (the size queries return 0). */
size_t fs_ssim_loss_saved_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t flags);
size_t fs_ssim_loss_scratch_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t flags);
int fs_ssim_loss_forward(int32_t B, int32_t C, int32_t H, int32_t W, int32_t flags, const float* pred, const float* gt,
                         double* ssim /*[B]*/, double* l1_mean /*[B]*/, void* saved /*NULL: no backward will follow*/,
                         void* scratch, void* stream);
int fs_ssim_loss_backward(int32_t B, int32_t C, int32_t H, int32_t W, int32_t flags, const float* pred, const float* gt,
                          const float* g_ssim /*[B] | NULL*/, const float* g_l1 /*[B] | NULL*/, const void* saved,
                          float* g_pred, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FREESPLAT_AMD_LOSS_H */
