/*
 * freesplat_amd_density.h -- adaptive density control (clone, split, prune) for the Gaussians of one scene, beside
 * freesplat_amd_optim.h: the entry points freesplat_amd.refine.GaussianAdam.accumulate / densify / reset_opacity call.
 *
 * Same rules as the other headers: plain device pointers + sizes + a hipStream_t (passed as void*), an int status
 * (FS_OK, FS_ERR_*), NO allocation, NO host synchronisation, stream-ordered, arguments validated before anything touches a
 * device, fs_last_error() text after a failed launch.  Dense row-major fp32 unless noted.  No atomics on floats and no
 * workgroup ever waits on another: every result has the same bits on every run and stream.
 *
 * A header of its own with a revision of its own (FS_DENSITY_API_VERSION): FS_ABI_VERSION, FS_LOSS_API_VERSION,
 * FS_OPTIM_API_VERSION and the symbol sets of the other three headers do not change.  The order of the five parameter arrays
 * in every pointer table is that of freesplat_amd_optim.h (FS_OPTIM_MEANS ... FS_OPTIM_SHS).
 */
#ifndef FREESPLAT_AMD_DENSITY_H
#define FREESPLAT_AMD_DENSITY_H

#include "freesplat_amd_optim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS_DENSITY_API_VERSION 1
int fs_density_api_version(void);

/* kind[i] of a source row, as fs_density_plan writes it */
#define FS_DENSITY_DROPPED 0 /* no output row */
#define FS_DENSITY_KEPT 1    /* one output row: a bit copy of parameters and moments */
#define FS_DENSITY_CLONE 2   /* two output rows: the original with its moments, a copy with zero moments */
#define FS_DENSITY_SPLIT 3   /* two output rows: child 0, child 1, both with zero moments */

/* indices into totals[4] */
#define FS_DENSITY_N_OUT 0
#define FS_DENSITY_N_CLONED 1
#define FS_DENSITY_N_SPLIT 2
#define FS_DENSITY_N_DROPPED 3

/* One elementwise launch over the statistics of a view.  For every row with radii[i] > 0:
 *   grad_accum[i] += sqrtf(gx * gx + gy * gy),  (gx, gy) = g_means2D[3 i], g_means2D[3 i + 1]   (every operation rounded on its own)
 *   denom[i]      += 1.0f
 *   max_radii[i]   = max(max_radii[i], (float)radii[i])
 * A row with radii[i] <= 0 is neither read (its gradient may hold anything, NaN included) nor written.
 *   g_means2D [N,3]: the rasterizer's gradient of means2D (NDC units); radii int32 [N]; grad_accum, denom, max_radii float [N],
 *   updated in place.
 * N == 0: FS_OK, nothing launched.  N < 0 or a NULL pointer: FS_ERR_INVALID_ARG. */
int fs_density_accumulate(int32_t N, const float* g_means2D, const int32_t* radii, float* grad_accum, float* denom,
                          float* max_radii, void* stream);

/* Bytes of scratch fs_density_plan needs for N source rows (0 for N <= 0).  The scratch need not be initialised. */
size_t fs_density_plan_scratch_bytes(int32_t N);

/* Classify every source row and exclusive-scan the per-row output counts: three launches (per-workgroup counts, one
 * workgroup that scans the block sums, per-workgroup scan + scatter).  With s_max = max(scales[i, :]) the rules are, in order,
 *   hot   = denom[i] > 0 && grad_accum[i] >= grad_threshold * denom[i]      (one fp32 product; no division; never seen: not hot)
 *   split = hot && s_max > dense_scale
 *   clone = hot && !split
 *   drop  = opacities[i] < min_opacity
 *        || (!split && max_screen_size > 0 && max_radii[i] > max_screen_size)
 *        || (prune_scale > 0 && s_max > (split ? child_prune_scale : prune_scale))
 * and the row emits 0 output rows if dropped, 2 if cloned or split, 1 otherwise.  The thresholds arrive rounded to float by
 * the caller; the kernel only compares.  child_prune_scale is (float)(1.6 * prune_scale): a split parent is dropped exactly
 * when its children (scales / 1.6) would be too large in world space, and its screen radius is not tested (its children have
 * not been seen yet).  This is the set 3DGS's clone -> split -> prune sequence leaves, in one pass.
 *   reads:  grad_accum, denom, max_radii float [N]; scales [N,3], opacities [N] (the ACTIVATED values the optimizer holds).
 *   writes: kind uint8 [N] (FS_DENSITY_*); offset uint32 [N] (exclusive scan of the output counts: the outputs of source row
 *           i are rows offset[i] and offset[i] + 1, so the row order is stable); src uint32 [2 N], of which the first n_out
 *           entries are written: src[o] = (2 i + j) | (split ? 2^31 : 0) for output row o = offset[i] + j (bit 31 is free:
 *           N < 2^30); totals int32 [4] in device memory = {n_out, n_cloned, n_split, n_dropped},
 *           counted by kind; scratch (fs_density_plan_scratch_bytes(N)).
 * N == 0: FS_OK, nothing launched (totals is not written).  N < 0, N >= 2^30, a NULL pointer, or a threshold that is negative
 * or NaN (+inf is allowed: grad_threshold = +inf plans a prune-only pass): FS_ERR_INVALID_ARG. */
int fs_density_plan(int32_t N, const float* grad_accum, const float* denom, const float* max_radii, const float* scales,
                    const float* opacities, float grad_threshold, float dense_scale, float min_opacity, float max_screen_size,
                    float prune_scale, float child_prune_scale, uint8_t* kind, uint32_t* offset, uint32_t* src /*[2N]*/,
                    int32_t* totals /*[4]*/, void* scratch, void* stream);

/* Move the five raw arrays and both moments of N source rows into N_out destination rows, in ONE launch that is driven by the
 * OUTPUT: destination row o takes source row (src[o] & (2^31 - 1)) >> 1 -- the second output of that row if src[o] & 1, a child
 * of a split if src[o] & 2^31 -- so writes are dense, reads are monotone in the source, and src[] is all the kernel reads of the
 * plan.  Per kind of the source row:
 *   kept   parameters and moments copied bit for bit
 *   clone  [original: parameters and moments copied | copy: parameters copied, moments zero]
 *   split  [child 0 | child 1]: rotation, logit and SH copied, moments zero,
 *          log_scale = log_scale - logf(1.6f) per component,
 *          mean      = mean + R(q / |q|) (s * z),  s = exp(log_scale) of the parent (the bits of fs_gaussian_activate), R as
 *                      rasterizer.build_cov3d defines it, z = three standard normals
 * and out_scales [N_out,3] / out_opacities [N_out] receive the activation of the NEW raw values by the device functions
 * fs_gaussian_activate uses (same raw value -> same bits).  fp32, every operation rounded on its own.
 *
 * z comes from a stateless counter-based generator, a pure function of (seed, source row, child, word) in 32-bit unsigned
 * arithmetic (wrapping), independent of the launch geometry:
 *   fmix(h):  h ^= h >> 16;  h *= 0x85EBCA6B;  h ^= h >> 13;  h *= 0xC2B2AE35;  h ^= h >> 16
 *   bits(seed, row, child, word) = fmix(fmix(fmix(seed ^ 0x9E3779B9) ^ row) + 0x9E3779B1 * (8 * child + word + 1))
 *   u(word) = ((float)(bits >> 8) + 0.5f) * 2^-24          (fp32: the sum rounds to even above 2^23, so u lies in (0, 1])
 *   z[c]    = sqrtf(-2 logf(u(2 c))) * cosf(6.2831855f * u(2 c + 1)),  c = 0, 1, 2                 (Box-Muller in fp32)
 *
 *   p_src, exp_avg_src, exp_avg_sq_src: host tables of FS_OPTIM_ARRAYS device pointers, N rows each, read only.
 *   p_dst, exp_avg_dst, exp_avg_sq_dst: host tables of FS_OPTIM_ARRAYS device pointers, N_out rows each, every element written.
 *   src uint32 [>= N_out]: as fs_density_plan wrote it.  N_out is passed by the host (totals[0] read back):
 *   no row at or beyond N_out is written whatever the plan holds, and an entry of src that names a row >= N writes zeros.
 * Arrays whose row is a multiple of 16 bytes (rotations, SH with M = 4 or 16) move with 16-byte loads and stores where the
 * pointers are 16-byte aligned; the other arrays take 16-byte stores (aligned destination) and 4-byte loads, since a
 * compaction shifts their rows by an arbitrary number of floats; unaligned pointers and array tails take 4-byte accesses.
 * N == 0 or N_out == 0: FS_OK, nothing launched.  N < 0, N_out < 0, N_out > 2 N (N > 0), M not in {1, 4, 9, 16},
 * 3 M N >= 2^31 or 3 M N_out >= 2^31, a NULL table, table entry, src, out_scales or out_opacities: FS_ERR_INVALID_ARG. */
int fs_density_apply(int32_t N, int32_t M, int32_t N_out, const uint32_t* src, const float* const* p_src,
                     const float* const* exp_avg_src, const float* const* exp_avg_sq_src, float* const* p_dst,
                     float* const* exp_avg_dst, float* const* exp_avg_sq_dst, float* out_scales, float* out_opacities,
                     uint32_t seed, void* stream);

/* One elementwise launch: logits[i] = min(logits[i], limit) with limit = (float)log(max_opacity / (1 - max_opacity)) formed in
 * double precision on the host; both opacity moments of every row set to 0; out_opacities [N] rewritten from the new logits.
 * N == 0: FS_OK, nothing launched.  N < 0, a NULL pointer, max_opacity outside (0, 1) or NaN: FS_ERR_INVALID_ARG. */
int fs_density_reset_opacity(int32_t N, double max_opacity, float* logits, float* exp_avg, float* exp_avg_sq,
                             float* out_opacities, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FREESPLAT_AMD_DENSITY_H */
