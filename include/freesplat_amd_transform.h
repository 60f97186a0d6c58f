/*
 * freesplat_amd_transform.h -- similarity transforms of Gaussian scenes in libfreesplat_hip.so (MI355X / gfx950): the
 * per-transform table (scale, rotation, translation, quaternion and the spherical-harmonics rotation blocks), the SH
 * rotation, and the transform of means, scales, rotations, covariances and harmonics with its backward, beside
 * freesplat_amd.h, freesplat_amd_loss.h, freesplat_amd_optim.h, freesplat_amd_density.h, freesplat_amd_depthloss.h,
 * freesplat_amd_normals.h, freesplat_amd_exposure.h and freesplat_amd_mvdepth.h.
 *
 * Same rules as the other headers: plain device pointers + sizes + a hipStream_t (passed as void*), an int status
 * (FS_OK, FS_ERR_*), NO allocation, NO host synchronisation, stream-ordered and hipGraph-capturable, arguments validated
 * before anything touches a device, fs_last_error() text after a failed launch.  Dense row-major fp32 unless noted.
 *
 * A header of its own with a revision of its own (FS_TRANSFORM_API_VERSION): the symbol sets and revisions of the other
 * eight headers do not change.  A binding checks fs_transform_api_version() next to the other eight.
 */
#ifndef FREESPLAT_AMD_TRANSFORM_H
#define FREESPLAT_AMD_TRANSFORM_H

#include "freesplat_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS_TRANSFORM_API_VERSION 1
int fs_transform_api_version(void);

/* ------------------------------------------------------------------------------------ *
 * The table of a transform                                                               *
 * ------------------------------------------------------------------------------------ */

/* A transform T = (s, R, t), s > 0, R a proper rotation, maps x to s R x + t.  Row v of a table holds, as fp32:
 *   [FS_TRANSFORM_S]         s
 *   [FS_TRANSFORM_R  .. +9)  R, row-major
 *   [FS_TRANSFORM_T  .. +3)  t
 *   [FS_TRANSFORM_Q  .. +4)  q_R = (w, x, y, z), the unit quaternion of R with w >= 0
 *   [FS_TRANSFORM_D1 .. +9)  D_1, row-major 3 x 3
 *   [FS_TRANSFORM_D2 .. +25) D_2, row-major 5 x 5
 *   [FS_TRANSFORM_D3 .. +49) D_3, row-major 7 x 7         (83 floats of SH blocks, 100 floats per row)
 * D_l(R) is the matrix with b_l(R d) = D_l(R) b_l(d) for every unit d, b_l being the 2l + 1 functions of band l of the
 * basis the rasterizer evaluates (freesplat_amd.h: the real SH of 3DGS, with its constants and signs, coefficients
 * l^2 .. (l+1)^2 - 1).  D_0 = 1 is not stored.
 *
 * fs_transform_prepare: xf [V,3,4], row v = (s R | t) of transform v.  One launch.  Everything is derived in fp64 from the fp32
 * entries of xf and rounded once: s = cbrt(det(s R)), R = the rotation nearest to (s R) / s (its polar factor; three steps of
 * Newton's iteration X <- (X + X^-T) / 2, which leaves a matrix that is a rotation to 2^-24 one to fp64 roundoff), q_R from R
 * (the candidate with the largest component, normalised, sign chosen for w >= 0), and
 *   D_l = 4 pi  sum_k w_k  b_l(R d_k) b_l(d_k)^T
 * over the 26 nodes d_k of the degree-7 Lebedev rule (6 axes, weight 1/21; 12 edge midpoints, 4/105; 8 corners, 9/280; the
 * weights sum to 1).  The products b_l,i b_l,j are polynomials of degree <= 6, which the rule integrates exactly, and the
 * basis is orthonormal on the sphere, so the sum IS D_l up to fp64 rounding.  The table is written in full; nothing checks
 * that xf is a similarity (a sheared or reflected xf gives a table that is not a rotation's: the caller's contract). */
#define FS_TRANSFORM_S 0
#define FS_TRANSFORM_R 1
#define FS_TRANSFORM_T 10
#define FS_TRANSFORM_Q 13
#define FS_TRANSFORM_D1 17
#define FS_TRANSFORM_D2 26
#define FS_TRANSFORM_D3 51
#define FS_TRANSFORM_TABLE_FLOATS 100
int fs_transform_prepare(int32_t V, const float* xf /*[V,3,4]*/, float* table /*[V,FS_TRANSFORM_TABLE_FLOATS]*/, void* stream);

/* ------------------------------------------------------------------------------------ *
 * Applying it                                                                            *
 * ------------------------------------------------------------------------------------ */

/* flags */
#define FS_TRANSFORM_SH_CHANNEL_MAJOR 1   /* shs are [N,3,M] (the adapter's harmonics); default [N,M,3] (the rasterizer's shs) */
#define FS_TRANSFORM_SH_TRANSPOSE 2       /* fs_sh_rotate only: apply D_l^T, the backward of the rotation and its inverse */
#define FS_TRANSFORM_QUAT_XYZW 4          /* rotations are (x, y, z, w) (the adapter's); default (w, x, y, z) */
#define FS_TRANSFORM_COV_FULL 8           /* cov is [N,3,3]; default [N,6] = (xx, xy, xz, yy, yz, zz) */

/* N Gaussians, M in {1, 4, 9, 16} SH coefficients per colour channel, V table rows.  ids [N] int64 in device memory names the
 * table row of each Gaussian; NULL means row 0 for all and requires V == 1.  The ids are never read on the host.  A Gaussian
 * whose id lies outside [0, V) is copied through bit for bit in every array and makes no kernel read or write outside the
 * arrays.  Every *_out may be the same pointer as its *_in (in place; the same bits as out of place); apart from that the
 * arrays must not overlap.
 *
 * fs_sh_rotate, band l of colour channel c of a Gaussian, c_j = coefficient l^2 + j, D = D_l of the Gaussian's row:
 *   out_i = fma(D[i][2l], c_2l, ... fma(D[i][1], c_1, D[i][0] * c_0))             (with FS_TRANSFORM_SH_TRANSPOSE: D[j][i])
 * and out_0 = c_0 for the band l = 0.
 *
 * fs_gaussians_transform_forward, with (s, R, t, q) of the Gaussian's row, E = R, p = q:
 *   means      r_i = fma(E[i][2], m_2, fma(E[i][1], m_1, E[i][0] * m_0)),   out_i = fma(s, r_i, t_i)
 *   scales     out_i = s * scale_i
 *   rotations  the Hamilton product p (x) g, g the Gaussian's quaternion (any norm; the norm is preserved):
 *                out_w = fma(-p_z, g_z, fma(-p_y, g_y, fma(-p_x, g_x, p_w * g_w)))
 *                out_x = fma(-p_z, g_y, fma( p_y, g_z, fma( p_x, g_w, p_w * g_x)))
 *                out_y = fma( p_z, g_x, fma( p_y, g_w, fma(-p_x, g_z, p_w * g_y)))
 *                out_z = fma( p_z, g_w, fma(-p_y, g_x, fma( p_x, g_y, p_w * g_z)))
 *   cov        S the 3 x 3 matrix (the symmetric one of the six stored entries, or the nine given), s2 = s * s:
 *                T[i][k] = fma(E[i][2], S[2][k], fma(E[i][1], S[1][k], E[i][0] * S[0][k]))
 *                out[i][j] = s2 * fma(T[i][2], E[j][2], fma(T[i][1], E[j][1], T[i][0] * E[j][0]))
 *              (six form: the entries i <= j)
 *   shs        as fs_sh_rotate with D
 * Opacities do not change under a similarity and have no argument.
 *
 * fs_gaussians_transform_backward maps the gradients of the outputs to the gradients of the inputs with the transposed linear
 * maps -- s R^T g, s g, conj(q) (x) g, s^2 R^T G R, D^T g -- through the same chains with E = R^T, p = conj(q) = (q_w, -q_x,
 * -q_y, -q_z), D[j][i], and out_i = s * r_i for the means.  For the six-entry covariance the result is the derivative with
 * respect to the six stored entries: the chains run on K = (g_xx, g_xy / 2, g_xz / 2, g_yy, g_yz / 2, g_zz) and the
 * off-diagonal results are doubled (both steps exact).  The gradient with respect to the transform itself (s, R, t) is not
 * computed here: fs_sim3_tangent (freesplat_amd_pose.h) contracts the inputs of the forward and the input gradients of this
 * backward with the generators of Sim(3), which is that gradient in the tangent space at the transform.
 *
 * Each array is optional: a NULL *_in skips it, and its *_out is then neither read nor written.  A non-NULL *_in needs a
 * non-NULL *_out.  All five NULL is FS_ERR_INVALID_ARG.
 *
 * Memory: a thread owns four consecutive Gaussians in the geometry arrays (and one or four in shs, by M), a run of floats
 * that starts at a multiple of 16 bytes from the array's base: arrays whose base is 16-byte aligned go through 16-byte
 * loads and stores, any other array and the last, partial run through dword accesses with a bound check.  The path changes
 * nothing about an element's arithmetic, so the bits are the same at any 4-byte alignment.  No atomics, no scratch memory,
 * no workgroup waits on another: the same bits on every run and stream.
 *
 * N, V <= 0, M not in {1, 4, 9, 16}, a NULL required pointer, ids NULL with V != 1, unknown flag bits: FS_ERR_INVALID_ARG. */
int fs_sh_rotate(int32_t N, int32_t M, int32_t V, int32_t flags, const float* sh_in, const float* table,
                 const int64_t* ids /*[N] | NULL*/, float* sh_out, void* stream);
int fs_gaussians_transform_forward(int32_t N, int32_t M, int32_t V, int32_t flags, const float* table, const int64_t* ids,
                                   const float* means_in /*[N,3] | NULL*/, const float* scales_in /*[N,3] | NULL*/,
                                   const float* rotations_in /*[N,4] | NULL*/, const float* cov_in /*[N,6] or [N,3,3] | NULL*/,
                                   const float* shs_in /*[N,M,3] or [N,3,M] | NULL*/, float* means_out, float* scales_out,
                                   float* rotations_out, float* cov_out, float* shs_out, void* stream);
int fs_gaussians_transform_backward(int32_t N, int32_t M, int32_t V, int32_t flags, const float* table, const int64_t* ids,
                                    const float* g_means_out, const float* g_scales_out, const float* g_rotations_out,
                                    const float* g_cov_out, const float* g_shs_out, float* g_means_in, float* g_scales_in,
                                    float* g_rotations_in, float* g_cov_in, float* g_shs_in, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FREESPLAT_AMD_TRANSFORM_H */
