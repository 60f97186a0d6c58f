/*
 * freesplat_amd_mvdepth.h -- the multi-view depth consistency loss and the scale-invariant depth loss of libfreesplat_hip.so
 * (MI355X / gfx950), forward and backward, beside freesplat_amd.h, freesplat_amd_loss.h, freesplat_amd_optim.h,
 * freesplat_amd_density.h, freesplat_amd_depthloss.h, freesplat_amd_normals.h and freesplat_amd_exposure.h.
 *
 * Same rules as the other headers: plain device pointers + sizes + a hipStream_t (passed as void*), an int status
 * (FS_OK, FS_ERR_*), NO allocation, NO host synchronisation, stream-ordered and hipGraph-capturable, arguments validated
 * before anything touches a device, fs_last_error() text after a failed launch.  Dense row-major fp32 unless noted.
 *
 * A header of its own with a revision of its own (FS_MVDEPTH_API_VERSION): the symbol sets and revisions of the other seven
 * headers do not change.  A binding checks fs_mvdepth_api_version() next to the other seven.
 */
#ifndef FREESPLAT_AMD_MVDEPTH_H
#define FREESPLAT_AMD_MVDEPTH_H

#include "freesplat_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS_MVDEPTH_API_VERSION 1
int fs_mvdepth_api_version(void);

#define FS_MVDEPTH_MAX_SOURCES 16 /* K */

/* ------------------------------------------------------------------------------------ *
 * Multi-view depth term and scale-invariant term (DESIGN.md "Multi-view depth loss")     *
 * ------------------------------------------------------------------------------------ */

/* depth, gt, alpha, g_depth, g_alpha [B,H,W]; alpha NULL: no alpha (then g_alpha NULL).
 *   E  = depth, or depth / max(alpha, alpha_floor)
 *   V0 = isfinite(gt) & gt > min_depth & gt < max_depth; a source sample S is valid under the same three tests.
 *
 * Sources, one of two layouts:
 *   src_index NULL:  src_depth [B,K,Hs,Ws], source k of view b is map b * K + k                       (S_pool is ignored)
 *   src_index [B,K]: int32 in device memory, src_depth [S_pool,Hs,Ws]; source k of view b is map src_index[b,k].  An index
 *                    outside [0, S_pool) makes the pair contribute sum 0 and count 0 (residual NaN) and forms no address.
 *                    The indices are never read on the host.
 * pairs [B,K,3,4]: row-major [A | t] of the pair, A = (K_s T_s<-w T_w<-c)[:, :3] K_c^-1, t = (K_s T_s<-w T_w<-c)[:, 3].
 *
 * For pixel (x, y) of view b and source k, with a = A (x, y, 1)^T:
 *   q = gt * a + t, z = q[2], z' = z + 1e-8, (u, v) = (q[0], q[1]) / z' if |z| > 1e-8 else (q[0], q[1])            (fp32)
 *   ix = rint(u), iy = rint(v) (half to even); S = src[iy, ix] if 0 <= ix < Ws and 0 <= iy < Hs, else not visible
 *   visible  = V0 & valid(S) & z' > 0 & z' < occlusion * S
 *   z_p'     = E * a[2] + t[2] + 1e-8;  selected = visible & isfinite(z_p') & z_p' > 0;  r = log z_p' - log S
 *   sum[b,k] = sum over the selected pixels of |r|, cnt[b,k] = their number (exact)
 *   residual [B,K,H,W] (optional): r, NaN where the pixel is not selected; every element is written.
 * The gather location depends on gt alone; z_p' and r are formed in fp64 from the fp32 operands, r is rounded once to fp32
 * (the value the residual map holds) and the sums add those values in fp64: sum[b,k] is the fp64 sum of |residual[b,k]|.
 *
 * Backward: g_sum [B,K] fp32 is the cotangent of sum;
 *   g_E = sum_k g_sum[b,k] sgn(r) a[2] / z_p' over the sources that select the pixel, then, with alpha,
 *   g_depth = g_E / max(alpha, alpha_floor), g_alpha = -g_depth E where alpha > alpha_floor, else 0; without, g_depth = g_E.
 * Every element of g_depth (and g_alpha) is written; a pixel no source selects receives exactly 0.  The backward recomputes
 * everything from the inputs: the forward saves nothing.
 *
 * Scale-invariant term, over P = V0 & isfinite(E) & E > 0 with d = log gt - log E:
 *   s1[b] = sum d, s2[b] = sum d^2, n[b] = |P| (exact);  backward: g_E = -(g_s1[b] + 2 d g_s2[b]) / E on P, exactly 0 elsewhere.
 *
 * Sums: fp64, in a fixed order -- a thread's pixels in index order, a fixed tree per workgroup, one row of partials per
 * workgroup in `scratch`, the rows of a (view, source) added in index order by one workgroup of a second launch.  No float
 * atomics, no workgroup waits on another.  A workgroup owns a fixed number of consecutive pixels of one view, so a view's
 * results have the same bits in any batch, on every run and stream, and for arrays at any 4-byte alignment (16-byte accesses
 * where a plane's base allows, dword accesses otherwise, the same arithmetic either way).
 *   scratch: fs_mvdepth_scratch_bytes(B, K, H, W) bytes (K = 0: what the scale-invariant forward needs; the size for K >= 2
 *   serves it too), free for reuse once the work has run; its contents need no initialisation.  The backwards need none.
 *
 * B, H, W, Hs, Ws, K <= 0, S_pool <= 0 with src_index given, a NULL required pointer, alpha NULL with g_alpha given or the
 * reverse, a NaN min_depth / max_depth / occlusion, an alpha_floor that is not positive and finite: FS_ERR_INVALID_ARG.
 * K > FS_MVDEPTH_MAX_SOURCES, H * W or Hs * Ws beyond 2^31 - 1, a workgroup count beyond 2^31 - 1: FS_ERR_UNSUPPORTED.
 * The size query returns 0 for either. */
size_t fs_mvdepth_scratch_bytes(int32_t B, int32_t K, int32_t H, int32_t W);
int fs_mv_depth_forward(int32_t B, int32_t K, int32_t H, int32_t W, int32_t Hs, int32_t Ws, int32_t S_pool, const float* depth,
                        const float* gt, const float* alpha /*| NULL*/, const float* src_depth,
                        const int32_t* src_index /*[B,K] | NULL*/, const float* pairs /*[B,K,3,4]*/, float occlusion,
                        float min_depth, float max_depth, float alpha_floor, double* sum /*[B,K]*/, double* cnt /*[B,K]*/,
                        float* residual /*[B,K,H,W] | NULL*/, void* scratch, void* stream);
int fs_mv_depth_backward(int32_t B, int32_t K, int32_t H, int32_t W, int32_t Hs, int32_t Ws, int32_t S_pool, const float* depth,
                         const float* gt, const float* alpha /*| NULL*/, const float* src_depth,
                         const int32_t* src_index /*[B,K] | NULL*/, const float* pairs, float occlusion, float min_depth,
                         float max_depth, float alpha_floor, const float* g_sum /*[B,K]*/, float* g_depth,
                         float* g_alpha /*| NULL*/, void* stream);
int fs_si_depth_forward(int32_t B, int32_t H, int32_t W, const float* depth, const float* gt, const float* alpha /*| NULL*/,
                        float min_depth, float max_depth, float alpha_floor, double* s1 /*[B]*/, double* s2 /*[B]*/,
                        double* n /*[B]*/, void* scratch, void* stream);
int fs_si_depth_backward(int32_t B, int32_t H, int32_t W, const float* depth, const float* gt, const float* alpha /*| NULL*/,
                         float min_depth, float max_depth, float alpha_floor, const float* g_s1 /*[B]*/,
                         const float* g_s2 /*[B]*/, float* g_depth, float* g_alpha /*| NULL*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FREESPLAT_AMD_MVDEPTH_H */
