/*
 * freesplat_amd_exposure.h -- per-view exposure compensation of libfreesplat_hip.so (MI355X / gfx950): the affine colour op,
 * its backward and the least-squares affine colour fit, beside freesplat_amd.h, freesplat_amd_loss.h, freesplat_amd_optim.h,
 * freesplat_amd_density.h, freesplat_amd_depthloss.h and freesplat_amd_normals.h.
 *
 * Same rules as the other headers: plain device pointers + sizes + a hipStream_t (passed as void*), an int status
 * (FS_OK, FS_ERR_*), NO allocation, NO host synchronisation, stream-ordered and hipGraph-capturable, arguments validated
 * before anything touches a device, fs_last_error() text after a failed launch.  Dense row-major fp32 unless noted.
 *
 * A header of its own with a revision of its own (FS_EXPOSURE_API_VERSION): the symbol sets and revisions of the other six
 * headers do not change.  A binding checks fs_exposure_api_version() next to the other six.
 */
#ifndef FREESPLAT_AMD_EXPOSURE_H
#define FREESPLAT_AMD_EXPOSURE_H

#include "freesplat_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS_EXPOSURE_API_VERSION 1
int fs_exposure_api_version(void);

/* ------------------------------------------------------------------------------------ *
 * Per-view affine colour transform: apply, its backward, and the least-squares fit       *
 * ------------------------------------------------------------------------------------ */

/* image, out, g_out, g_image, pred, target [B,3,H,W]; params, g_params [V,3,4]: row c of view v is (A[c,0], A[c,1], A[c,2],
 * b[c]), the identity is [I | 0].  view_ids [B] int64 in device memory maps a batch entry to its view; NULL means entry b
 * uses view b and requires B == V.  The ids are never read on the host.  P = H * W, p a pixel, v = view_ids[b]:
 *
 *   out[b,c,p]      = fma(A[v,c,2], x2, fma(A[v,c,1], x1, fma(A[v,c,0], x0, b[v,c])))          x_k = image[b,k,p]
 *   g_image[b,k,p]  = fma(A[v,2,k], g2, fma(A[v,1,k], g1, A[v,0,k] * g0))                       g_c = g_out[b,c,p]
 *   g_params[v,c,k] = sum over the entries b with view_ids[b] == v, over p, of g_out[b,c,p] * image[b,k,p]   (k < 3)
 *   g_params[v,c,3] = the same sum of g_out[b,c,p]
 *
 * No clamp, no masking: non-finite values propagate as plain arithmetic does.  An entry whose id lies outside [0, V) is passed
 * through (out = image and g_image = g_out, bit for bit), contributes to no parameter gradient, and makes no kernel read or
 * write outside its arrays.  g_params is written in full (not accumulated into): exactly 0 for a view that no entry
 * references; entries that share a view are added in batch-index order.  g_image and g_params are optional: NULL selects a
 * kernel that neither computes nor writes it (both NULL: FS_ERR_INVALID_ARG).  `image` is required only with g_params,
 * `scratch` likewise.
 *
 * fs_exposure_fit: mask [B,H,W] uint8 (nonzero = use) or NULL.  A pixel is valid iff the mask admits it and its six colour
 * values are finite; an invalid pixel never enters consumed arithmetic.  Per view v, over the valid pixels of all entries with
 * that id, with X = (x0, x1, x2, 1) of pred and y of target:
 *   M = sum X X^T (10 distinct sums), R = sum X y^T (12 sums), cnt = M[3,3], lambda = ridge * cnt,
 *   P solves (M + lambda I4) P = R + lambda [I3; 0]  by Cholesky,  params[v] = P^T,  count[v] = cnt,  solved[v] = 1.
 * cnt == 0, or a pivot that is not positive and finite (possible only with ridge == 0): params[v] = the identity exactly and
 * solved[v] = 0.  params [V,3,4] fp32, count [V] int64, solved [V] uint8 are written in full.
 *
 * Arithmetic: the per-pixel chains above in fp32 (explicit fused multiply-adds in that order, whatever path loads the pixel);
 * every sum in fp64 -- products of fp32 values formed in fp64 (exact), per-thread sums in a fixed order, a fixed tree per
 * workgroup, one row of partials per workgroup in `scratch`, the rows of a view added in a fixed order by one workgroup -- and
 * rounded once to fp32; the 4 x 4 solve in fp64, rounded once.  No float atomics, no workgroup waits on another: the same bits
 * on every run and stream, for any batch an entry comes in, and for arrays at any 4-byte alignment.
 *   scratch: fs_exposure_scratch_bytes(B, H, W) bytes, free for reuse once the work has run; its contents need no initialisation.
 *
 * B, V, H, W <= 0, a NULL required pointer, view_ids NULL with B != V, a ridge that is negative or not finite:
 * FS_ERR_INVALID_ARG (the size query returns 0).  H * W beyond 2^31 - 1 (the kernels' 32-bit pixel index) or a workgroup
 * count beyond 2^31 - 1: FS_ERR_UNSUPPORTED (the size query returns 0). */
size_t fs_exposure_scratch_bytes(int32_t B, int32_t H, int32_t W);
int fs_exposure_apply_forward(int32_t B, int32_t V, int32_t H, int32_t W, const float* image, const float* params /*[V,3,4]*/,
                              const int64_t* view_ids /*[B] | NULL: entry b uses view b*/, float* out, void* stream);
int fs_exposure_apply_backward(int32_t B, int32_t V, int32_t H, int32_t W, const float* image /*NULL allowed without g_params*/,
                               const float* params, const int64_t* view_ids, const float* g_out, float* g_image /*| NULL*/,
                               float* g_params /*[V,3,4] | NULL*/, void* scratch /*NULL allowed without g_params*/, void* stream);
int fs_exposure_fit(int32_t B, int32_t V, int32_t H, int32_t W, const float* pred, const float* target,
                    const uint8_t* mask /*[B,H,W] | NULL*/, const int64_t* view_ids, double ridge, float* params /*[V,3,4]*/,
                    int64_t* count /*[V]*/, uint8_t* solved /*[V]*/, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FREESPLAT_AMD_EXPOSURE_H */
