/*
 * freesplat_ext_raycast.h -- ray casting of a TSDF volume into per-view depth, normal and colour maps of libfreesplat_hip.so
 * (MI355X / gfx950).  An extension header: it stands beside the eleven freesplat_amd*.h headers, whose symbol sets and revisions
 * do not change, and has a revision of its own (FS_RAYCAST_API_VERSION) that a binding checks after theirs.
 *
 * Same rules as the other headers: plain device pointers + sizes + a hipStream_t (passed as void*), an int status
 * (FS_OK, FS_ERR_*), NO allocation, stream-ordered, arguments validated before anything touches a device, fs_last_error()
 * text after a failed launch.  Dense row-major fp32.  Every output element is written by exactly one thread: no atomics, no
 * workgroup waits on another, the same bits on every run and stream and at every 4-byte alignment of the arrays.  Nothing is
 * read on the host: the call is hipGraph-capturable.
 */
#ifndef FREESPLAT_EXT_RAYCAST_H
#define FREESPLAT_EXT_RAYCAST_H

#include "freesplat_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS_RAYCAST_API_VERSION 1
int fs_raycast_api_version(void);

/* The pixels one workgroup of 256 threads owns (a wavefront owns an 8 x 8 tile of them). */
#define FS_RAYCAST_TILE 16
#define FS_RAYCAST_MAX_REFINE 32
#define FS_RAYCAST_MAX_STEPS (1 << 20)

/* The volume is the one of freesplat_amd_tsdf.h: tsdf, weight [Z,Y,X], optional color [3,Z,Y,X]; grid point (i, j, k) lies at
 * origin + voxel_size * (i, j, k).  cam_to_world [V,3,4] = rows (A_c0 A_c1 A_c2 c_c), c = x, y, z: the top three rows of the
 * camera-to-world matrices as given, no inverse is formed.  intrinsics [V,4] = (fx, fy, cx, cy), integer pixel coordinates being
 * pixel centres (the convention of freesplat_amd_normals.h).
 *
 * Per view and pixel (px, py), in fp32 with every operation rounded on its own (correctly rounded / and sqrt), in exactly this
 * association.  min2(a, b) = (a < b or b is NaN) ? a : b and max2(a, b) = (a > b or b is NaN) ? a : b: fminf / fmaxf with the
 * choice they leave open fixed (a NaN is dropped; of a +0 / -0 pair the second operand is returned).
 *
 *   1. ray      dx = ((float)px - cx) / fx,  dy = ((float)py - cy) / fy.  The march parameter s is z-depth: what the rasterizer
 *               outputs and fs_tsdf_integrate consumes.
 *   2. grid     o_c = (c_c - origin_c) / voxel_size,  d_c = ((A_c0 * dx + A_c1 * dy) + A_c2) / voxel_size,
 *               g_c(s) = o_c + s * d_c,  L = sqrt((d_x^2 + d_y^2) + d_z^2)   (voxels per unit of depth)
 *   3. interval s0 = min_depth, s1 = max_depth; per axis c = x, y, z in that order with n = X, Y, Z:
 *               a = (0 - o_c) / d_c,  b = ((float)(n - 1) - o_c) / d_c,  s0 = max2(s0, min2(a, b)),  s1 = min2(s1, max2(a, b)).
 *               The ray is dead unless s0 <= s1 (a NaN makes it dead).  A volume with a dimension of 1 has no cell: every ray
 *               is dead.  A dead ray reads nothing.
 *   4. sample   at s: per axis fl = floorf(g_c); fi = fl > 0 ? fl : 0 (NaN gives 0); fi = fi < n - 2 ? fi : n - 2; the cell index
 *               is (int)fi -- formed on the floats, so non-finite and huge values form no address --, t_c = g_c - fi.
 *               Corner q of the cell has offset (q & 1, q >> 1 & 1, q >> 2 & 1).  The sample is OBSERVED iff all eight corner
 *               weights are >= min_weight (a NaN weight is not).  lerp(a, b, t) = a + t * (b - a).  The value is
 *               f = lerp_z(lerp_y(lerp_x(c0, c1), lerp_x(c2, c3)), lerp_y(lerp_x(c4, c5), lerp_x(c6, c7))).
 *   5. march    s = s0, no previous sample, at most max_steps samples (an integer counter: the bound that ends the kernel).
 *               Sample at s.  If the previous and this sample are both observed, !(f_prev < 0) and f < 0: stop with the bracket
 *               (sa, fa, sb, fb) = (s_prev, f_prev, s, f).  Otherwise the sample becomes the previous one and
 *               s = s + step / L with step = fmaxf(step_min, relax * (|f| * (trunc / voxel_size))) for an observed sample (a NaN
 *               value takes step_min and never counts as negative) and relax * (trunc / voxel_size) for an unobserved one; the
 *               ray ends without a hit when !(s <= s1).
 *   6. refine   `refine` times: sm = sa + (fa / (fa - fb)) * (sb - sa); sample at sm; observed and f < 0: (sb, fb) = (sm, f);
 *               observed otherwise: (sa, fa) = (sm, f); unobserved: nothing changes.
 *   7. outputs  depth [V,H,W] = sa + (fa / (fa - fb)) * (sb - sa), 0 where there is no hit (the rasterizer's convention: a hole
 *               to every depth consumer).  One more sample at that depth.  From its eight corners the gradient of the trilinear
 *               field, differences first, then the lerps of step 4 over the other two axes in the order x, y, z:
 *                 G_x = lerp_z(lerp_y(c1 - c0, c3 - c2), lerp_y(c5 - c4, c7 - c6))
 *                 G_y = lerp_z(lerp_x(c2 - c0, c3 - c1), lerp_x(c6 - c4, c7 - c5))
 *                 G_z = lerp_y(lerp_x(c4 - c0, c5 - c1), lerp_x(c6 - c2, c7 - c3))
 *               m_j = -((A_xj * G_x + A_yj * G_y) + A_zj * G_z) for j = 0, 1, 2,  len = sqrt((m_0^2 + m_1^2) + m_2^2),
 *               normals [V,3,H,W] = m_j / len: camera space, the convention of fs_depth_normals_forward (a fronto-parallel
 *               surface seen from the front gives (0, 0, +1)).  The pixel is VALID iff the ray hit, the last sample is observed
 *               and 0 < len < inf.  normals are NaN in all three channels of a pixel that is not valid (what gt_normals treats
 *               as missing); out_color [V,3,H,W] is the value of step 4 per colour plane at the last sample, 0 where the pixel
 *               is not valid; steps [V,H,W] is the number of march samples the ray took (0 for a dead ray).
 *
 * A workgroup owns FS_RAYCAST_TILE x FS_RAYCAST_TILE pixels of one view; the views go into the grid as one flat workgroup index.
 * The results do not depend on which optional outputs are asked for, nor on the other views of the call.
 *
 * X, Y, Z, V, H, W <= 0, a NULL tsdf / weight / cam_to_world / intrinsics / depth, out_color without color, a NaN or infinite
 * origin, a voxel_size / trunc / step_min / relax that is not positive and finite, a NaN or negative min_depth, a NaN max_depth,
 * a min_weight that is not positive (or NaN), refine outside 0 .. FS_RAYCAST_MAX_REFINE, max_steps outside
 * 1 .. FS_RAYCAST_MAX_STEPS: FS_ERR_INVALID_ARG.  X * Y * Z or H * W beyond 2^31 - 1, or more than 2^31 - 1 workgroups:
 * FS_ERR_UNSUPPORTED.  Linear indices are 64-bit. */
int fs_tsdf_raycast(int32_t X, int32_t Y, int32_t Z, float ox, float oy, float oz, float voxel_size, float trunc,
                    const float* tsdf, const float* weight, const float* color /*[3,Z,Y,X] | NULL*/, int32_t V, int32_t H,
                    int32_t W, const float* cam_to_world /*[V,3,4]*/, const float* intrinsics /*[V,4]*/, float min_depth,
                    float max_depth, float min_weight, float step_min, float relax, int32_t refine, int32_t max_steps,
                    float* depth /*[V,H,W]*/, float* normals /*[V,3,H,W] | NULL*/, float* out_color /*[V,3,H,W] | NULL*/,
                    int32_t* steps /*[V,H,W] | NULL*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FREESPLAT_EXT_RAYCAST_H */
