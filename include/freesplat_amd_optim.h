/*
 * freesplat_amd_optim.h -- parameter-update entry points of libfreesplat_hip.so (MI355X / gfx950), beside freesplat_amd.h
 * and freesplat_amd_loss.h.
 *
 * Same rules as the main header: plain device pointers + sizes + a hipStream_t (passed as void*), an int status
 * (FS_OK, FS_ERR_*), NO allocation, NO host synchronisation, stream-ordered and hipGraph-capturable, arguments validated
 * before anything touches a device, fs_last_error() text after a failed launch.  Dense row-major fp32 unless noted.
 *
 * The declarations live in a header of their own with a revision of their own (FS_OPTIM_API_VERSION): FS_ABI_VERSION,
 * FS_LOSS_API_VERSION and the symbol sets of the other two headers do not change.  A binding checks fs_optim_api_version()
 * next to fs_abi_version().
 */
#ifndef FREESPLAT_AMD_OPTIM_H
#define FREESPLAT_AMD_OPTIM_H

#include "freesplat_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS_OPTIM_API_VERSION 1
int fs_optim_api_version(void);

/* ------------------------------------------------------------------------------------ *
 * Fused Adam step over the parameters of one scene's Gaussians (per-scene refinement)   *
 * ------------------------------------------------------------------------------------ */

/* The five parameter arrays, in the order of every p / g / exp_avg / exp_avg_sq pointer table below, and what the
 * rasterizer consumes of each (its FS_RASTER_SCALE_ROT inputs):
 *   FS_OPTIM_MEANS      means      [N,3]    as stored
 *   FS_OPTIM_SCALES     log-scales [N,3]    scale   = exp(x)
 *   FS_OPTIM_ROTATIONS  rotations  [N,4]    as stored (the rasterizer normalises the quaternion itself)
 *   FS_OPTIM_OPACITIES  logits     [N]      opacity = 1 / (1 + exp(-x))
 *   FS_OPTIM_SHS        shs        [N,M,3]  as stored, M in {1, 4, 9, 16}
 * and the six learning-rate groups, the order of lr_dev[6]: the SH array is two groups, coefficient 0 (FS_OPTIM_LR_SH_DC)
 * and coefficients 1 .. M-1 (FS_OPTIM_LR_SH_REST). */
#define FS_OPTIM_MEANS 0
#define FS_OPTIM_SCALES 1
#define FS_OPTIM_ROTATIONS 2
#define FS_OPTIM_OPACITIES 3
#define FS_OPTIM_SHS 4
#define FS_OPTIM_ARRAYS 5

#define FS_OPTIM_LR_MEANS 0
#define FS_OPTIM_LR_SCALES 1
#define FS_OPTIM_LR_ROTATIONS 2
#define FS_OPTIM_LR_OPACITIES 3
#define FS_OPTIM_LR_SH_DC 4
#define FS_OPTIM_LR_SH_REST 5
#define FS_OPTIM_LR_GROUPS 6

/* out_scales [N,3] = exp(log_scales), out_opacities [N] = 1 / (1 + exp(-logits)): the activation of the raw parameters, by
 * the device functions fs_gaussian_adam_step uses (same raw value -> same bits).  N == 0: FS_OK, nothing launched.  N < 0 or a
 * NULL pointer: FS_ERR_INVALID_ARG. */
int fs_gaussian_activate(int32_t N, const float* log_scales, const float* logits, float* out_scales, float* out_opacities,
                         void* stream);

/* One Adam step (torch.optim.Adam without weight decay or amsgrad) over the five arrays in ONE launch, then a one-thread
 * launch that advances the step counter.  Per element, with g the gradient with respect to the raw parameter,
 *   m = beta1 m + (1 - beta1) g,   v = beta2 v + (1 - beta2) g^2,
 *   p = p - (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps)),        bc1 = 1 - beta1^t, bc2 = 1 - beta2^t,
 * in fp32; bc1, bc2, lr / bc1 and sqrt(bc2) are formed in double precision on the device (one lane per workgroup) from
 * t = step_dev[0] + 1, and 1 - beta in double precision on the host.
 *   p, exp_avg, exp_avg_sq: host tables of FS_OPTIM_ARRAYS device pointers, updated in place.
 *   g: host table of the rasterizer's gradient arrays (g_means, g_scales, g_rotations, g_opacities, g_shs), i.e. gradients with
 *     respect to the ACTIVATED values: the kernel applies g_log_scale = g_scale * scale and g_logit = g_opacity * o * (1 - o),
 *     with scale and o recomputed from the raw parameter before the update.  An entry may be NULL: that array is left
 *     untouched (p, exp_avg, exp_avg_sq and its share of out_scales / out_opacities); not all five.
 *   visible: NULL, or int32 [N] (the rasterizer's radii; a row is visible where the value is > 0).  A row that is not visible
 *     is skipped whole: its gradients are not used (they may hold anything), its p, exp_avg, exp_avg_sq, out_scales and
 *     out_opacities are not written, its moments do not decay; t is global all the same (sparse Adam).
 *   lr_dev: float [FS_OPTIM_LR_GROUPS] in device memory, read by the kernel: a stream-ordered write changes a rate.
 *   step_dev: int32 [1] in device memory, the number of steps taken so far; read as t - 1 and incremented on the stream.
 *   out_scales [N,3], out_opacities [N]: the activation of the updated raw values, written by the same launch.
 * Pointers that are 16-byte aligned (p, g, both moments and the activated output of an array) take 16-byte accesses; an array
 * with any other pointer is processed with 4-byte accesses.  No atomics, no scratch: the result has the same bits on every
 * run and stream.  3 M N must stay below 2^31 (element indices are 32-bit).
 * N == 0: FS_OK, nothing launched.  N < 0, 3 M N >= 2^31, M not in {1, 4, 9, 16}, a NULL table, a NULL p / exp_avg /
 * exp_avg_sq entry, lr_dev, step_dev, out_scales or out_opacities, all five g entries NULL, beta1 or beta2 outside [0, 1)
 * or eps < 0 (or any of them NaN): FS_ERR_INVALID_ARG. */
int fs_gaussian_adam_step(int32_t N, int32_t M, float* const* p, const float* const* g, float* const* exp_avg,
                          float* const* exp_avg_sq, const int32_t* visible /*[N] | NULL*/, const float* lr_dev /*[6]*/,
                          int32_t* step_dev /*[1]*/, double beta1, double beta2, double eps, float* out_scales,
                          float* out_opacities, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FREESPLAT_AMD_OPTIM_H */
