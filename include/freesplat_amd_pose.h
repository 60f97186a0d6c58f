/*
 * freesplat_amd_pose.h -- gradients with respect to a similarity or a camera pose in libfreesplat_hip.so (MI355X / gfx950):
 * the contraction of per-Gaussian values and gradients with the generators of Sim(3), beside freesplat_amd.h,
 * freesplat_amd_loss.h, freesplat_amd_optim.h, freesplat_amd_density.h, freesplat_amd_depthloss.h, freesplat_amd_normals.h,
 * freesplat_amd_exposure.h, freesplat_amd_mvdepth.h and freesplat_amd_transform.h.
 *
 * Same rules as the other headers: plain device pointers + sizes + a hipStream_t (passed as void*), an int status
 * (FS_OK, FS_ERR_*), NO allocation, NO host synchronisation, stream-ordered and hipGraph-capturable, arguments validated
 * before anything touches a device, fs_last_error() text after a failed launch.  Dense row-major fp32 unless noted.
 *
 * A header of its own with a revision of its own (FS_POSE_API_VERSION): the symbol sets and revisions of the other nine
 * headers do not change.  A binding checks fs_pose_api_version() next to the other nine.
 */
#ifndef FREESPLAT_AMD_POSE_H
#define FREESPLAT_AMD_POSE_H

#include "freesplat_amd.h"
#include "freesplat_amd_transform.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS_POSE_API_VERSION 1
int fs_pose_api_version(void);

/* A tangent vector of Sim(3) is xi = (u, omega, sigma), 7 numbers in that order: the infinitesimal similarity
 *   x -> x + sigma x + omega x x + u.
 * It moves the arrays of a Gaussian scene by
 *   means      d mu    = sigma mu + omega x mu + u
 *   scales     d s     = sigma s
 *   rotations  d q     = 1/2 (0, omega) (x) q          (Hamilton product; a quaternion of any norm)
 *   cov        d Sigma = 2 sigma Sigma + [omega]x Sigma - Sigma [omega]x
 *   shs        d c_l   = sum_k omega_k G_{l,k} c_l     (band l of every colour channel; G_0 = 0)
 * with G_{l,k} = d D_l(exp(theta [e_k]x)) / d theta at 0, D_l the blocks of freesplat_amd_transform.h: constant antisymmetric
 * (2l+1) x (2l+1) matrices of the basis the rasterizer evaluates.
 *
 * fs_sim3_tangent contracts the gradients g_* of a scalar L with respect to the arrays with those motions: row v of `out` is
 * dL / d xi over the Gaussians whose id is v,
 *   tau_u       = sum g_mu
 *   tau_omega,k = sum [ (mu x g_mu)_k + 1/2 g_q . (e_k (x) q) + <G_Sigma, [e_k]x Sigma - Sigma [e_k]x>
 *                       + sum_{l, channel} g_c,l^T G_{l,k} c_l ]
 *   tau_sigma   = sum [ mu . g_mu + s . g_s + 2 <G_Sigma, Sigma> ]
 * For the six-entry covariance g_cov is the gradient with respect to the six stored entries and the six entries of d Sigma are
 * contracted with it (the convention of fs_gaussians_transform_backward).
 *
 * Uses: with the INPUTS of fs_gaussians_transform_forward and the input gradients of its backward, the result is the gradient
 * of L with respect to xi in T Exp(xi) at xi = 0 (the transform's own gradient in the right tangent space at T); with the
 * arrays a view was rendered from and the gradients the rasterizer returned, it is the gradient with respect to a motion of
 * the scene, which is minus that of the camera.
 *
 * Arithmetic: every product and sum is formed in fp64 from the fp32 inputs.  A thread owns four consecutive Gaussians and adds
 * their terms in a fixed order (Gaussian by Gaussian: means, scales, rotations, cov, shs), a workgroup of 256 threads reduces
 * its 1024 Gaussians in a fixed fp64 tree and writes one row of seven partial sums per id to `scratch`, and a second launch
 * with one workgroup per id adds the rows in a fixed order.  No float atomics, no workgroup waits on another: the same bits
 * on every run and stream.  Arrays whose base is 16-byte aligned are read with 16-byte loads, any other array and the last,
 * partial run with dword loads and a bound check; the values and their order are the same, so the bits do not depend on the
 * alignment.  The partial sums of an id depend only on the positions and values of the Gaussians with that id: a Gaussian with
 * another id, or an id outside [0, V), contributes nothing and is not read where its whole run of four is skipped.
 *
 * fs_sim3_tangent_scratch_bytes: the bytes fs_sim3_tangent needs at `scratch` (0 for invalid sizes).
 *
 * fs_sim3_sh_generators: a HOST function (no device is touched).  Writes the 3 x 83 doubles of the generators the kernel uses:
 * out[k * 83 + o] for k = x, y, z and o running over the row-major blocks G_{1,k} (9), G_{2,k} (25), G_{3,k} (49) -- the
 * layout of the D_1, D_2, D_3 blocks of a table row.  FS_ERR_INVALID_ARG for NULL.
 *
 * fs_sim3_tangent: N Gaussians, M in {1, 4, 9, 16} SH coefficients per colour channel, V ids.  `flags` are the layout bits
 * FS_TRANSFORM_SH_CHANNEL_MAJOR, FS_TRANSFORM_QUAT_XYZW and FS_TRANSFORM_COV_FULL (freesplat_amd_transform.h, the same values).
 * ids [N] int64 in device memory names the row of each Gaussian; NULL means row 0 for all and requires V == 1.  The ids are
 * never read on the host.  Each (values, gradient) pair is optional and is given or omitted together; an omitted pair adds
 * nothing.  The one exception: tau_u needs no values, so g_means may be given with means NULL -- the means then add tau_u only.
 * out [V,7] fp64 is written in full (zeros for an id without a Gaussian).  Two launches.
 *
 * N <= 0, M not in {1, 4, 9, 16}, V outside 1 .. FS_SIM3_MAX_ROWS, unknown flag bits (FS_TRANSFORM_SH_TRANSPOSE among them),
 * ids NULL with V != 1, values without their gradient, a gradient other than g_means without its values, all five gradients
 * NULL, out or scratch NULL, scratch_bytes below fs_sim3_tangent_scratch_bytes(N, V): FS_ERR_INVALID_ARG. */
#define FS_SIM3_MAX_ROWS 64
#define FS_SIM3_TANGENT_DIM 7
#define FS_SIM3_SH_GENERATOR_DOUBLES 83
size_t fs_sim3_tangent_scratch_bytes(int32_t N, int32_t V);
int fs_sim3_sh_generators(double* out /*[3,83], host*/);
int fs_sim3_tangent(int32_t N, int32_t M, int32_t V, int32_t flags, const int64_t* ids /*[N] | NULL*/,
                    const float* means /*[N,3] | NULL*/, const float* scales /*[N,3] | NULL*/, const float* rotations /*[N,4] | NULL*/,
                    const float* cov /*[N,6] or [N,3,3] | NULL*/, const float* shs /*[N,M,3] or [N,3,M] | NULL*/,
                    const float* g_means, const float* g_scales, const float* g_rotations, const float* g_cov, const float* g_shs,
                    double* out /*[V,7]*/, void* scratch, size_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FREESPLAT_AMD_POSE_H */
