/*
 * freesplat_amd_normals.h -- surface normals from depth and the normals loss of libfreesplat_hip.so (MI355X / gfx950), beside
 * freesplat_amd.h, freesplat_amd_loss.h, freesplat_amd_optim.h, freesplat_amd_density.h and freesplat_amd_depthloss.h.
 *
 * Same rules as the other headers: plain device pointers + sizes + a hipStream_t (passed as void*), an int status
 * (FS_OK, FS_ERR_*), NO allocation, NO host synchronisation, stream-ordered and hipGraph-capturable, arguments validated
 * before anything touches a device, fs_last_error() text after a failed launch.  Dense row-major fp32 unless noted.
 *
 * A header of its own with a revision of its own (FS_NORMALS_API_VERSION): the symbol sets and revisions of the other five
 * headers do not change.  A binding checks fs_normals_api_version() next to the other five.
 */
#ifndef FREESPLAT_AMD_NORMALS_H
#define FREESPLAT_AMD_NORMALS_H

#include "freesplat_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS_NORMALS_API_VERSION 1
int fs_normals_api_version(void);

/* ------------------------------------------------------------------------------------ *
 * Depth -> camera-space surface normals, and the cosine loss between two normal maps     *
 * ------------------------------------------------------------------------------------ */

/* depth, alpha, gt_depth [B,H,W]; gt_normals, normals, g_normals [B,3,H,W]; intrinsics [B,4] = (fx, fy, cx, cy) in pixels, in
 * device memory (trusted: fx, fy finite and non-zero).  alpha may be NULL.
 *   E  = depth                                   (alpha NULL)
 *      = depth / max(alpha, alpha_floor)         (dE/dalpha = -depth / alpha^2 where alpha > alpha_floor, else 0)
 *   E is valid iff isfinite(E) && E > 0 (fs_depth_normals_*: && E > min_depth && E < max_depth); gt_depth is valid iff
 *   isfinite && > min_depth && < max_depth.  An invalid value never enters arithmetic that is consumed.
 *   sigma > 0: S = the separable 5 x 5 blur of the depth, w_k ~ exp(-k^2 / (2 sigma^2)), k = -2..2, normalised to 1 in double
 *   and rounded once to fp32, replicate-clamped coordinates, valid iff all 25 clamped taps are valid.  sigma == 0: S = the
 *   depth itself (no smoothing; the kernels for it carry the small halos, they do not run the blur with a unit kernel).
 *   P(px, py) = S(px, py) * ((px - cx) / fx, (py - cy) / fy, 1)
 *   Gx = Sobel_x(P) / 8, Gy = Sobel_y(P) / 8 per component, replicate-clamped, valid iff all nine clamped taps are valid
 *   n  = (Gx x Gy) / max(|Gx x Gy|, 1e-12)       (a fronto-parallel plane gives (0, 0, +1))
 *   target t: the same chain on gt_depth, or gt_normals as given (valid iff its three components are finite; not renormalised)
 *   sum[b] = sum over M_b of 0.5 (1 - n . t), cnt[b] = |M_b|, M_b = the pixels of view b where n and t are both valid.
 *
 * fs_depth_normals_forward writes n, NaN in all three channels where it is invalid.  fs_normals_loss_forward writes sum and
 * cnt [B] as double and no normal map: per-pixel arithmetic is fp32 up to the Sobel vectors and fp64 from the cross product on,
 * the sums fp64 in a fixed order without float atomics, so a view's values are the same bits whatever the batch, the stream
 * or the run.  Exactly one of gt_depth / gt_normals is given.
 *   scratch: fs_normals_scratch_bytes(B, H, W) bytes (one partial row per workgroup), free for reuse once the work has run.
 *
 * The backward calls recompute everything from the inputs (nothing is saved by the forward) and write g_depth [B,H,W] and,
 * when alpha was given, g_alpha [B,H,W] in full (they do not rely on zeroed buffers): a gather, every element written by
 * exactly one thread, no float atomics.  fs_normals_loss_backward takes the per-view cotangents g_sum [B] (fp32, device memory);
 * fs_depth_normals_backward takes g_normals, whose values at invalid pixels are ignored.  A pixel whose E is invalid receives
 * exactly 0.  The target gets no gradient.
 *
 * Sizes <= 0, H * W or the workgroup count beyond 2^31 - 1, a NULL required pointer, both or neither target, alpha without
 * g_alpha in a backward, a NaN min_depth / max_depth, an alpha_floor that is not a positive finite number, a sigma that is
 * negative or not finite: FS_ERR_INVALID_ARG (the size query returns 0).  sigma == 0 is the "no smoothing" encoding. */
size_t fs_normals_scratch_bytes(int32_t B, int32_t H, int32_t W);
int fs_depth_normals_forward(int32_t B, int32_t H, int32_t W, const float* depth, const float* alpha /*NULL: E = depth*/,
                             const float* intrinsics /*[B,4]*/, float sigma /*0: no smoothing*/, float min_depth,
                             float max_depth, float alpha_floor, float* normals /*[B,3,H,W]*/, void* stream);
int fs_depth_normals_backward(int32_t B, int32_t H, int32_t W, const float* depth, const float* alpha, const float* intrinsics,
                              float sigma, float min_depth, float max_depth, float alpha_floor,
                              const float* g_normals /*[B,3,H,W]*/, float* g_depth, float* g_alpha /*NULL iff alpha is NULL*/,
                              void* stream);
int fs_normals_loss_forward(int32_t B, int32_t H, int32_t W, const float* depth, const float* alpha /*NULL: E = depth*/,
                            const float* intrinsics /*[B,4]*/, const float* gt_depth /*[B,H,W] | NULL*/,
                            const float* gt_normals /*[B,3,H,W] | NULL*/, float sigma /*0: no smoothing*/, float min_depth,
                            float max_depth, float alpha_floor, double* sum /*[B]*/, double* cnt /*[B]*/, void* scratch,
                            void* stream);
int fs_normals_loss_backward(int32_t B, int32_t H, int32_t W, const float* depth, const float* alpha, const float* intrinsics,
                             const float* gt_depth, const float* gt_normals, float sigma, float min_depth, float max_depth,
                             float alpha_floor, const float* g_sum /*[B]*/, float* g_depth,
                             float* g_alpha /*NULL iff alpha is NULL*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FREESPLAT_AMD_NORMALS_H */
