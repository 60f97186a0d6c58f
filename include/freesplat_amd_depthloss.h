/*
 * freesplat_amd_depthloss.h -- depth-supervision loss of libfreesplat_hip.so (MI355X / gfx950), beside freesplat_amd.h,
 * freesplat_amd_loss.h, freesplat_amd_optim.h and freesplat_amd_density.h.
 *
 * Same rules as the other headers: plain device pointers + sizes + a hipStream_t (passed as void*), an int status
 * (FS_OK, FS_ERR_*), NO allocation, NO host synchronisation, stream-ordered and hipGraph-capturable, arguments validated
 * before anything touches a device, fs_last_error() text after a failed launch.  Dense row-major fp32 unless noted.
 *
 * A header of its own with a revision of its own (FS_DEPTHLOSS_API_VERSION): the symbol sets and revisions of the other four
 * headers do not change.  A binding checks fs_depthloss_api_version() next to the other four.
 */
#ifndef FREESPLAT_AMD_DEPTHLOSS_H
#define FREESPLAT_AMD_DEPTHLOSS_H

#include "freesplat_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS_DEPTHLOSS_API_VERSION 1
int fs_depthloss_api_version(void);

/* ------------------------------------------------------------------------------------ *
 * Point term (log-L1 or L1) + multi-scale gradient term, forward and backward           *
 * ------------------------------------------------------------------------------------ */

/* `mode` is exactly one of the two point terms. */
#define FS_DEPTH_LOSS_LOG_L1 1
#define FS_DEPTH_LOSS_L1 2
#define FS_DEPTH_LOSS_MAX_SCALES 6

/* depth, gt, alpha [B,H,W]; alpha may be NULL.  S = number of pyramid levels, 1..6.
 *   E  = depth                                   (alpha NULL)
 *      = depth / max(alpha, alpha_floor)         (dE/dalpha = -depth / alpha^2 where alpha > alpha_floor, else 0)
 *   V0 = isfinite(gt) && gt > min_depth && gt < max_depth; an invalid gt (NaN, +-inf, 0, negative, ...) is never used in
 *        arithmetic, and no consumed value depends on an invalid pixel.
 *   point term over P = V0 && E > 0 (LOG_L1) or P = V0 (L1):
 *        point_sum[b] = sum_P |log E - log gt|  resp.  sum_P |E - gt|,     point_cnt[b] = |P|
 *   pyramid of linear depth, level 0 = (E, gt, V0), level s+1 of size ceil(H_s / 2) x ceil(W_s / 2):
 *        X_{s+1}[i,j] = 1/16 sum_{a,b in -1..1} k_a k_b X_s[2i+a, 2j+b], k = (1,2,1), taps outside the level contribute 0;
 *        V_{s+1}[i,j] = every tap inside the level is valid
 *   gradient term at every level: g_x = 1/8 Sobel_x, g_y = 1/8 Sobel_x^T with replicate clamping, M_s = all nine clamped taps
 *   valid,
 *        grad_sum[b,s] = sum_{M_s} |g_x(E_s) - g_x(gt_s)| + |g_y(E_s) - g_y(gt_s)|,   grad_cnt[b,s] = 2 |M_s|
 * All four outputs are double.  Per-pixel arithmetic is fp32 on the residual E - gt (every step above is linear), the sums
 * fp64 in a fixed order without atomics: a view's values are the same bits whatever the batch, the stream or the run.
 *   saved:   NULL (no backward will follow), or fs_depth_loss_saved_bytes(B, H, W, S) bytes that receive levels 1..S-1 of the
 *            residual pyramid (fp32, an invalid element stored as NaN).  Opaque to the caller; about 1.33 bytes per pixel.
 *   scratch: fs_depth_loss_scratch_bytes(B, H, W, S) bytes, free for reuse once the call's work has run.
 *
 * fs_depth_loss_backward writes g_depth [B,H,W] and, when alpha was given, g_alpha [B,H,W] in full (it does not rely on
 * zeroed buffers) for the per-view cotangents g_point [B] (of point_sum) and g_grad [B,S] (of grad_sum), both fp32 in
 * device memory; either may be NULL (that term is left out; `saved` is then not read for a NULL g_grad), not both.  A gather
 * from the top level down: every pixel of a level collects the Sobel contributions of its 3 x 3 neighbourhood and the
 * blur-pool contributions of the level above; no atomics, the same bits on every run.  sign(0) = 0.  A pixel with an
 * invalid gt receives exactly 0.  depth, gt, alpha, the scalars and the sizes must be those of the forward call that
 * filled `saved`.  scratch: fs_depth_loss_scratch_bytes(B, H, W, S) bytes.
 *
 * Sizes <= 0, S outside 1..6, a `mode` other than the two above, a NULL required pointer, a NaN min_depth / max_depth, an
 * alpha_floor that is not a positive finite number, alpha without g_alpha in the backward, or a g_grad without `saved`:
 * FS_ERR_INVALID_ARG (the size queries return 0). */
size_t fs_depth_loss_saved_bytes(int32_t B, int32_t H, int32_t W, int32_t S);
size_t fs_depth_loss_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t S);
int fs_depth_loss_forward(int32_t B, int32_t H, int32_t W, int32_t S, int32_t mode, const float* depth, const float* gt,
                          const float* alpha /*NULL: E = depth*/, float min_depth, float max_depth, float alpha_floor,
                          double* point_sum /*[B]*/, double* point_cnt /*[B]*/, double* grad_sum /*[B,S]*/,
                          double* grad_cnt /*[B,S]*/, void* saved /*NULL: no backward will follow*/, void* scratch,
                          void* stream);
int fs_depth_loss_backward(int32_t B, int32_t H, int32_t W, int32_t S, int32_t mode, const float* depth, const float* gt,
                           const float* alpha /*NULL: E = depth*/, float min_depth, float max_depth, float alpha_floor,
                           const float* g_point /*[B] | NULL*/, const float* g_grad /*[B,S] | NULL*/, const void* saved,
                           float* g_depth, float* g_alpha /*NULL iff alpha is NULL*/, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FREESPLAT_AMD_DEPTHLOSS_H */
