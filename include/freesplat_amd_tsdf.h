/*
 * freesplat_amd_tsdf.h -- volumetric TSDF fusion of depth maps and marching-tetrahedra mesh extraction of libfreesplat_hip.so
 * (MI355X / gfx950), beside freesplat_amd.h, freesplat_amd_loss.h, freesplat_amd_optim.h, freesplat_amd_density.h,
 * freesplat_amd_depthloss.h, freesplat_amd_normals.h, freesplat_amd_exposure.h, freesplat_amd_mvdepth.h,
 * freesplat_amd_transform.h and freesplat_amd_pose.h.
 *
 * Same rules as the other headers: plain device pointers + sizes + a hipStream_t (passed as void*), an int status
 * (FS_OK, FS_ERR_*), NO allocation, stream-ordered, arguments validated before anything touches a device, fs_last_error()
 * text after a failed launch.  Dense row-major fp32.  No float atomics, no workgroup waits on another: the same bits on every
 * run and stream.  fs_tsdf_integrate and fs_tsdf_mesh_plan / _emit read nothing on the host and are hipGraph-capturable; the
 * caller's read of fs_tsdf_mesh_plan's total between plan and emit is the only host synchronisation of an extraction.
 *
 * A header of its own with a revision of its own (FS_TSDF_API_VERSION): the symbol sets and revisions of the other ten
 * headers do not change.  A binding checks fs_tsdf_api_version() next to the other ten.
 */
#ifndef FREESPLAT_AMD_TSDF_H
#define FREESPLAT_AMD_TSDF_H

#include "freesplat_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS_TSDF_API_VERSION 1
int fs_tsdf_api_version(void);

/* Views of one fs_tsdf_integrate call.  A workgroup decides which views can touch its brick with one lane per view and keeps
 * the answer as one 64-bit ballot of a wavefront, walked in bit order: 64 views is what that word holds.  A caller with more
 * views makes several calls in order (freesplat_amd.tsdf does); the result is that of one call per view. */
#define FS_TSDF_MAX_VIEWS 64

/* The brick of grid points one workgroup of 256 threads owns (a thread owns FS_TSDF_BRICK_X / 8 = 4 consecutive x). */
#define FS_TSDF_BRICK_X 32
#define FS_TSDF_BRICK_Y 8
#define FS_TSDF_BRICK_Z 4
/* Consecutive linear cube indices one workgroup of the extraction owns. */
#define FS_TSDF_MESH_RUN 256

/* flags of fs_tsdf_integrate */
#define FS_TSDF_NO_BRICK_SKIP 1 /* every workgroup walks every view (measurements and tests: the results have the same bits) */

/* ------------------------------------------------------------------------------------ *
 * The volume (DESIGN.md "TSDF fusion")                                                  *
 * ------------------------------------------------------------------------------------ */

/* tsdf [Z,Y,X]: sdf / trunc in [-1, 1].  weight [Z,Y,X]: observations, capped at max_weight.  color [3,Z,Y,X]: optional planes,
 * present on every call for a volume or on none.  Grid point (i, j, k) lies at
 *   x = ox + voxel_size * (float)i,  y = oy + voxel_size * (float)j,  z = oz + voxel_size * (float)k      (one product, one sum)
 * and is a corner of the cubes the mesh is cut from.  Linear indices are 64-bit; X * Y * Z up to 2^31 - 1.
 *
 * fs_tsdf_integrate fuses the V views of the call into the volume in place, in ONE launch.  Per grid point, for v = 0 .. V - 1
 * in that order, in fp32 with every operation rounded on its own, in exactly this association:
 *   1. p_c = ((R_c0 * x + R_c1 * y) + R_c2 * z) + t_c for c = x, y, z, with world_to_cam [V,3,4] = rows (R_c0 R_c1 R_c2 t_c)
 *   2. skip the view unless p_z > near
 *   3. u = fx * (p_x / p_z) + cx,  v = fy * (p_y / p_z) + cy   with intrinsics [V,4] = (fx, fy, cx, cy); integer pixel
 *      coordinates are pixel centres (the convention of freesplat_amd_normals.h; the caller folds in its own)
 *      ix = rint(u), iy = rint(v), half to even; skip unless 0 <= ix < W and 0 <= iy < H, tested on the floats (NaN and huge
 *      values form no address)
 *   4. d = depth[v,iy,ix]; with alpha [V,H,W]: skip where alpha < alpha_min, else d = d / max(alpha, alpha_floor)
 *      (fmaxf: a NaN alpha gives the floor); skip unless isfinite(d) & d > min_depth & d < max_depth (holes: NaN, +-inf, 0, < 0)
 *   5. sdf = d - p_z                                                          (z-depth, what the rasterizer outputs)
 *   6. skip if sdf < -trunc; s = min(1, sdf / trunc)
 *   7. W' = W + 1;  tsdf = (tsdf * W + s) / W';  per colour plane c = (c * W + image[v,ch,iy,ix]) / W' with image [V,3,H,W];
 *      W = min(W', max_weight)
 * A grid point no view updates is not written.  The view table, the intrinsics and the maps are device memory and are never
 * read on the host.
 *
 * A workgroup skips a view whose every (grid point of the brick, view) pair provably fails step 2 or the range test of step 3:
 * it evaluates steps 1 - 3 with the same fp32 operations at the brick's eight corner grid points; every operation of those
 * steps is monotone in each of its operands, so the corner values bracket every point's, and a view is skipped only when the
 * bracket lies behind `near` or rounds to pixels off one side of the map.  The skip changes no result bit
 * (FS_TSDF_NO_BRICK_SKIP turns it off).
 *
 * Results have the same bits for arrays at any 4-byte alignment (16-byte accesses where the four points of a thread allow it,
 * dword accesses otherwise, the same arithmetic either way) and whether a view comes alone or among views that do not see
 * the volume.
 *
 * X, Y, Z, V, H, W <= 0, a NULL tsdf / weight / world_to_cam / intrinsics / depth, color without image or image without color,
 * a NaN or infinite origin, a NaN near / min_depth / max_depth / alpha_min, a voxel_size / trunc / max_weight / alpha_floor that
 * is not positive and finite, an unknown flag: FS_ERR_INVALID_ARG.  V > FS_TSDF_MAX_VIEWS, X * Y * Z or H * W beyond 2^31 - 1:
 * FS_ERR_UNSUPPORTED. */
int fs_tsdf_integrate(int32_t X, int32_t Y, int32_t Z, float ox, float oy, float oz, float voxel_size, float trunc,
                      float max_weight, float* tsdf, float* weight, float* color /*[3,Z,Y,X] | NULL*/, int32_t V, int32_t H,
                      int32_t W, const float* world_to_cam /*[V,3,4]*/, const float* intrinsics /*[V,4]*/,
                      const float* depth /*[V,H,W]*/, const float* alpha /*[V,H,W] | NULL*/, const float* image /*[V,3,H,W] | NULL*/,
                      float near, float min_depth, float max_depth, float alpha_min, float alpha_floor, int32_t flags,
                      void* stream);

/* ------------------------------------------------------------------------------------ *
 * Marching tetrahedra                                                                   *
 * ------------------------------------------------------------------------------------ */

/* Cube (i, j, k), i < X - 1, j < Y - 1, k < Z - 1, linear index (k (Y - 1) + j) (X - 1) + i, is live iff all eight corners have
 * weight >= min_weight.  Corner c has offset (c & 1, c >> 1 & 1, c >> 2 & 1).  A live cube is cut into the six Kuhn tetrahedra
 * {c0, c0 + e_a, c0 + e_a + e_b, c7}, tetrahedron t taking (a, b, .) = the t-th permutation of (0, 1, 2) in lexicographic order;
 * a tetrahedron's vertices are numbered 0 .. 3 in that order.  A vertex is inside iff tsdf < 0 (an exact 0, a -0 and a NaN are
 * outside); bit m of a tetrahedron's case is set iff its vertex m is inside.
 *
 * fs_tsdf_mt_table (a host function, no device): the 6 x 16 x 7 bytes (tet, case) -> (number of triangles, 6 edge codes); an
 * edge code is (A << 3) | B for the cube corners A < B of the cut edge; triangle k takes codes 3 k .. 3 k + 2.  One vertex o
 * against p < q < r: (op, oq, or).  Inside {a, b}, a < b, outside {c, d}, c < d: (ac, ad, bd), (ac, bd, bc).  Where that order
 * would make (B - A) x (C - A), with every cut at its edge's midpoint, point from the outside vertices' mean to the inside
 * vertices' mean, the triangle's last two entries are swapped: normals point into free space.  The winding is the table's,
 * never decided by arithmetic on the data.
 *
 * Cut point of an edge with grid points P0 (corner A) and P1 (corner B) -- A < B is also the order of their linear indices --
 * and values f0, f1:  t = f0 / (f0 - f1),  P = P0 + t * (P1 - P0) per component (the grid coordinates of above; fp32, every
 * operation rounded on its own); colour the same way.  An edge gives the same bits from every tetrahedron and cube sharing it.
 *
 * Output: a triangle soup vertices [T,3,3] (and colors [T,3,3] when the volume has colour) ordered by linear cube index, then
 * tetrahedron, then triangle.  Zero-area triangles (a cut on a grid point) are emitted like any other.
 *
 * fs_tsdf_mesh_plan: every workgroup counts the triangles of its FS_TSDF_MESH_RUN consecutive cubes, one workgroup scans the
 * counts; *total (int64, device memory) receives T.  fs_tsdf_mesh_emit: every workgroup derives its cubes' cases again and
 * writes its triangles from its offset; T is the total the caller read (a smaller T truncates the soup, nothing is written
 * beyond T triangles).  scratch: fs_tsdf_mesh_scratch_bytes(X, Y, Z) bytes, written by plan, read by emit, no initialisation;
 * it is per workgroup, not per cube.  T == 0: emit does nothing and the output pointers may be NULL.  A volume with a
 * dimension of 1 has no cube: T = 0.
 *
 * X, Y, Z <= 0, a NULL required pointer, color without colors or the reverse, a min_weight that is not positive (or NaN), a NaN
 * or infinite origin, a voxel_size that is not positive and finite, T < 0: FS_ERR_INVALID_ARG.  X * Y * Z beyond 2^31 - 1, or
 * 9 T beyond 2^31 - 1 (the float offsets of the soup are 32-bit): FS_ERR_UNSUPPORTED.  The size query returns 0 for either. */
int fs_tsdf_mt_table(uint8_t* table /*[6*16*7]*/);
size_t fs_tsdf_mesh_scratch_bytes(int32_t X, int32_t Y, int32_t Z);
int fs_tsdf_mesh_plan(int32_t X, int32_t Y, int32_t Z, const float* tsdf, const float* weight, float min_weight,
                      int64_t* total /*device*/, void* scratch, void* stream);
int fs_tsdf_mesh_emit(int32_t X, int32_t Y, int32_t Z, float ox, float oy, float oz, float voxel_size, const float* tsdf,
                      const float* weight, const float* color /*[3,Z,Y,X] | NULL*/, float min_weight, const void* scratch,
                      int64_t T, float* vertices /*[T,3,3]*/, float* colors /*[T,3,3] | NULL*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FREESPLAT_AMD_TSDF_H */
