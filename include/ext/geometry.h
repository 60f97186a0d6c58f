/*
 * ext/geometry.h -- exact nearest neighbours between point clouds on a uniform grid, with the reductions the 3D geometry metrics
 * need (accuracy, completeness, Chamfer distance, precision / recall / F-score at a threshold), of libfreesplat_hip.so
 * (MI355X / gfx950).  An add-on header: it lives under include/ext/, has a revision of its own (FS_GEOMETRY_API_VERSION) and is
 * bound and checked after the headers directly under include/ (freesplat_amd/_lib.py ADDON_HEADERS).
 *
 * Same rules as the other headers: plain device pointers + sizes + a hipStream_t (passed as void*, the last argument), an int
 * status (FS_OK, FS_ERR_*), NO allocation, stream-ordered, arguments validated before anything touches a device, fs_last_error()
 * text after a failed launch.  Dense row-major fp32 points [N, 3].  Every output element is written by exactly one thread: no
 * atomics, no workgroup waits on another, the same bits on every run and stream and at every 4-byte alignment of the point
 * arrays.  Nothing is read on the host: every call is hipGraph-capturable.
 *
 * THE GRID.  lo[3], cell > 0 and n[3] (1 <= n_c <= FS_NN_MAX_SIDE, n_x n_y n_z <= FS_NN_MAX_CELLS) describe a uniform grid.  The
 * cell of a point p, reference point or query alike, is per axis c, in fp32, every operation rounded on its own,
 *
 *     i_c = clamp(floor((p_c - lo_c) * inv_cell), 0, n_c - 1),      inv_cell = 1.0f / cell
 *
 * (the clamp is made on the floats, so a huge value forms no integer), and its key is (i_z n_y + i_y) n_x + i_x.  A point with a
 * NaN or infinite coordinate has no cell: its key is "none" = n_x n_y n_z, which sorts behind every cell.
 *
 * THE DEFINITION.  For a query q and a reference point r, d = q - r per axis and d2 = (d_x d_x + d_y d_y) + d_z d_z, in fp32 with
 * every operation rounded on its own (no contraction).  The nearest neighbour of q is the reference point with finite
 * coordinates of the smallest d2, of equal ones the one with the smallest original index.  It COUNTS iff d2 < +inf and
 * d2 <= max_dist2.  A query with a neighbour that counts gets (d2, that index); one without gets (+inf, -1); a query with a NaN or
 * infinite coordinate gets (NaN, -1).  So the outputs are defined bit for bit by a loop over the whole reference, and the grid
 * only decides how much of it a query looks at.
 */
#ifndef FREESPLAT_EXT_GEOMETRY_H
#define FREESPLAT_EXT_GEOMETRY_H

#include "../freesplat_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FS_GEOMETRY_API_VERSION 1
int fs_geometry_api_version(void);

#define FS_NN_MAX_SIDE 1024
#define FS_NN_MAX_CELLS (1 << 24)
#define FS_NN_MAX_THRESHOLDS 8
/* doubles of fs_nn_query's `sums`: the queries with finite coordinates, those with a neighbour that counts, the sum of
 * sqrt((double)d2) over the latter, then per threshold t the number of the latter with d2 <= tau2[t] (0 beyond n_tau).  The counts
 * are integers below 2^31 held in doubles: exact. */
#define FS_NN_SUM_FIELDS (3 + FS_NN_MAX_THRESHOLDS)
#define FS_NN_SUM_FINITE 0
#define FS_NN_SUM_WITHIN 1
#define FS_NN_SUM_DIST 2
#define FS_NN_SUM_TAU 3

/* keys [N] int32 = the cell keys of points [N, 3] (see above).  One thread per point.
 * N < 0, a NULL points / keys (with N > 0), a NaN or infinite lo, a cell outside [1e-30, 1e15] (so that inv_cell and
 * (FS_NN_MAX_SIDE cell)^2 are finite), a side outside 1 .. FS_NN_MAX_SIDE, more than FS_NN_MAX_CELLS cells: FS_ERR_INVALID_ARG.
 * N = 0: FS_OK, nothing is launched. */
int fs_nn_grid_keys(int32_t N, const float* points, float lo_x, float lo_y, float lo_z, float cell, int32_t n_x, int32_t n_y,
                    int32_t n_z, int32_t* keys, void* stream);

/* records [N] of 16 bytes (16-byte aligned) = (x, y, z, the bits of the int32 original index) of points[order[i]]: the reference in
 * the order of a stable sort of its keys (order = the sort's int64 permutation), so that the points of a cell, and of consecutive
 * cells along x, are one contiguous stream of 16-byte loads.  An order[i] outside 0 .. N - 1 reads nothing and gives the record
 * (NaN, NaN, NaN, -1).  N < 0, a NULL pointer (with N > 0), records not 16-byte aligned: FS_ERR_INVALID_ARG.  N = 0: FS_OK. */
int fs_nn_grid_gather(int32_t N, const float* points, const int64_t* order, void* records, void* stream);

/* Bytes of fs_nn_query's `scratch` for Nq queries (one row of FS_NN_SUM_FIELDS doubles per workgroup); 0 for Nq <= 0. */
size_t fs_nn_query_scratch_bytes(int32_t Nq);

/* ONE launch for the Nq queries, one thread per query, followed by a one-workgroup launch that adds the workgroups' rows when
 * `sums` is asked for.
 *
 *   records [N_records], cell_start [n_x n_y n_z + 1] int32: cell k owns records cell_start[k] .. cell_start[k + 1] - 1 (the first
 *       index of each key in the sorted keys; cell_start[cells] = the number of reference points that have a cell).  A range is
 *       clipped to 0 .. N_records before it is walked, so no content of cell_start forms an address outside records.
 *   query_order [Nq] int64 | NULL: thread i answers query query_order[i] (and writes ITS outputs), e.g. the permutation of a sort
 *       of the queries' own keys, which puts the queries of a wavefront into neighbouring cells.  An entry outside 0 .. Nq - 1
 *       answers nothing.  dist2 and index do not depend on it; `sums` is added in thread order, so its sum of distances is one
 *       fixed association per (Nq, query_order) and differs in the last bits between two orders.
 *   max_dist2: max_dist^2 formed in double and rounded to fp32, +inf for none; tau2 [n_tau] likewise, a HOST array read during
 *       the call.
 *
 * The search visits the cells around the query's own (clamped) cell by Chebyshev rings k = 0, 1, ..  After ring k is complete it
 * stops once b = (float)k - 1/64 > 0 and (best d2 <= (b cell)^2 or (b cell)^2 >= max_dist2), or when the ring has left the grid on
 * every side, or at k = FS_NN_MAX_SIDE (an integer bound).  Every point not yet visited lies at least k cells from the query (from
 * its projection onto the grid's box, for a query outside; a projection onto a convex set lengthens no distance into the set), and
 * 1/64 of a cell is the margin for the fp32 rounding of the two cell assignments (each at most ~2.4e-4 of a cell at 1024 cells
 * per side): what the search skips cannot win, so the outputs are those of the definition above.  With max_dist2 = +inf a far
 * outlier walks out to the grid's edge.
 *
 *   dist2 [Nq] fp32 | NULL, index [Nq] int32 | NULL, sums [FS_NN_SUM_FIELDS] doubles | NULL (with scratch of
 *   fs_nn_query_scratch_bytes(Nq), 8-byte aligned).  The sum's association: per workgroup of 256 threads fs_reduce.h's
 *   block_sum_waves, then the rows in index order strided over 256 threads and block_sum_waves again; it does not depend on
 *   which of dist2 / index are asked for.
 *
 * Nq < 0, N_records < 0, a NULL query / cell_start (with Nq > 0), NULL records with N_records > 0, records not 16-byte aligned,
 * the grid conditions of fs_nn_grid_keys, a NaN or negative max_dist2, n_tau outside 0 .. FS_NN_MAX_THRESHOLDS, a NULL tau2 with
 * n_tau > 0, a NaN tau2, sums without scratch: FS_ERR_INVALID_ARG.  Nq = 0: FS_OK, nothing is launched and nothing written. */
int fs_nn_query(int32_t Nq, const float* query, const int64_t* query_order, int32_t N_records, const void* records,
                const int32_t* cell_start, float lo_x, float lo_y, float lo_z, float cell, int32_t n_x, int32_t n_y, int32_t n_z,
                float max_dist2, int32_t n_tau, const float* tau2, float* dist2, int32_t* index, double* sums, void* scratch,
                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FREESPLAT_EXT_GEOMETRY_H */
