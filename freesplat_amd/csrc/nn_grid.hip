// nn_grid.hip -- exact nearest neighbours between point clouds on a uniform grid and the sums of the geometry metrics
// (include/ext/geometry.h; freesplat_amd.geometry_metrics).
//
//   Build: one thread per reference point writes its cell key (nn_keys_kernel); the caller sorts the keys (stable) and takes the
//   first index of every key; one thread per sorted slot gathers the point into a 16-byte record (x, y, z, original index), so a
//   cell -- and a run of cells along x, which are consecutive keys -- is one contiguous, 16-byte aligned stream.
//
//   Query: one thread per query walks Chebyshev rings of cells around the query's own cell.  A ring is visited row by row (fixed
//   z, y): a row on the ring's shell is ONE run of records (cells x0 .. x1), a row inside it is the two cells at x = cx -+ k.  Each
//   record is one 16-byte load; the best (d2, index) pair lives in two registers.  All loop bounds are integers (ring <= 1024,
//   rows inside the grid, records clipped to the array), so no content of an input array makes a loop endless or an address
//   outside its array.  No LDS besides the block sum's 4 x 11 doubles, no atomics, no scratch memory.
//
//   Sums: every thread contributes (finite, within, sqrt((double)d2), d2 <= tau2[t]) to fs_reduce.h's block_sum_waves; a
//   workgroup writes one row; finalize_rows_kernel adds the rows.
//
// Numerics: fp32, every operation rounded on its own (-ffp-contract=off); the sums in fp64 in a fixed association.
#include "fs_reduce.h"

#include <limits.h>
#include <math.h>

#include "../../include/ext/geometry.h"

namespace fs {

namespace {

constexpr int kNnF = FS_NN_SUM_FIELDS;
constexpr float kRingMargin = 1.0f / 64.0f;

struct NnGrid {
    float lo[3];
    float cell, inv_cell;
    int n[3];
};

struct NnQueryArgs {
    const float* query;
    const long long* order;
    const float4* rec;
    const int32_t* start;
    float* dist2;
    int32_t* index;
    double* rows;
    NnGrid g;
    float max_d2;
    float tau2[FS_NN_MAX_THRESHOLDS];
    int Nq, Nrec, n_tau;
};

__device__ __forceinline__ bool finite3(float x, float y, float z)
{
    return fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY;          // (NaN fails)
}

// the header's cell formula along one axis; the clamp is made on the floats
__device__ __forceinline__ int cell_axis(float p, float lo, float inv_cell, int n)
{
    float t = floorf((p - lo) * inv_cell);
    t = t > 0.0f ? t : 0.0f;
    const float m = (float)(n - 1);
    t = t < m ? t : m;
    return (int)t;
}

__global__ __launch_bounds__(kSumThreads) void nn_keys_kernel(int N, const float* __restrict__ pts, const NnGrid g, int32_t* __restrict__ keys)
{
    const int i = blockIdx.x * kSumThreads + threadIdx.x;
    if (i >= N) return;
    const float x = pts[3ll * i], y = pts[3ll * i + 1], z = pts[3ll * i + 2];
    int key = g.n[0] * g.n[1] * g.n[2];                                                 // "none"
    if (finite3(x, y, z)) {
        const int ix = cell_axis(x, g.lo[0], g.inv_cell, g.n[0]), iy = cell_axis(y, g.lo[1], g.inv_cell, g.n[1]),
                  iz = cell_axis(z, g.lo[2], g.inv_cell, g.n[2]);
        key = (iz * g.n[1] + iy) * g.n[0] + ix;
    }
    keys[i] = key;
}

__global__ __launch_bounds__(kSumThreads) void nn_gather_kernel(int N, const float* __restrict__ pts, const long long* __restrict__ order,
                                                                float4* __restrict__ rec)
{
    const int i = blockIdx.x * kSumThreads + threadIdx.x;
    if (i >= N) return;
    const long long o = order[i];
    float4 r = make_float4(NAN, NAN, NAN, __int_as_float(-1));
    if (o >= 0 && o < N) r = make_float4(pts[3 * o], pts[3 * o + 1], pts[3 * o + 2], __int_as_float((int)o));
    rec[i] = r;
}

// the records of cells c0 .. c1 (consecutive keys) against the query
__device__ __forceinline__ void scan_cells(const NnQueryArgs& a, int c0, int c1, float qx, float qy, float qz, float& best, int& bi)
{
    int s = a.start[c0], e = a.start[c1 + 1];
    s = s > 0 ? s : 0;
    e = e < a.Nrec ? e : a.Nrec;
    for (int j = s; j < e; ++j) {
        const float4 r = a.rec[j];
        const float dx = qx - r.x, dy = qy - r.y, dz = qz - r.z;
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        const int id = __float_as_int(r.w);
        if (d2 < best || (d2 == best && id < bi)) {
            best = d2;
            bi = id;
        }
    }
}

__global__ __launch_bounds__(kSumThreads) void nn_query_kernel(const NnQueryArgs a)
{
    __shared__ double s_red[kSumWaves * kNnF];
    const long long i = (long long)blockIdx.x * kSumThreads + threadIdx.x;
    long long qi = -1;
    if (i < a.Nq) {
        qi = a.order ? a.order[i] : i;
        if (qi < 0 || qi >= a.Nq) qi = -1;
    }
    double v[kNnF];
#pragma unroll
    for (int f = 0; f < kNnF; ++f) v[f] = 0.0;

    if (qi >= 0) {
        const float qx = a.query[3 * qi], qy = a.query[3 * qi + 1], qz = a.query[3 * qi + 2];
        const bool finite = finite3(qx, qy, qz);
        float best = INFINITY;
        int bi = INT_MAX;
        if (finite) {
            const int nx = a.g.n[0], ny = a.g.n[1], nz = a.g.n[2];
            const int cx = cell_axis(qx, a.g.lo[0], a.g.inv_cell, nx), cy = cell_axis(qy, a.g.lo[1], a.g.inv_cell, ny),
                      cz = cell_axis(qz, a.g.lo[2], a.g.inv_cell, nz);
            for (int k = 0; k <= FS_NN_MAX_SIDE; ++k) {
                const int x0 = max(cx - k, 0), x1 = min(cx + k, nx - 1);
                const int y0 = max(cy - k, 0), y1 = min(cy + k, ny - 1);
                const int z0 = max(cz - k, 0), z1 = min(cz + k, nz - 1);
                for (int z = z0; z <= z1; ++z) {
                    const bool zshell = z - cz == k || cz - z == k;
                    for (int y = y0; y <= y1; ++y) {
                        const int row = (z * ny + y) * nx;
                        if (zshell || y - cy == k || cy - y == k) {
                            scan_cells(a, row + x0, row + x1, qx, qy, qz, best, bi);
                        } else {                                                        // (k > 0 here)
                            if (cx - k >= 0) scan_cells(a, row + cx - k, row + cx - k, qx, qy, qz, best, bi);
                            if (cx + k <= nx - 1) scan_cells(a, row + cx + k, row + cx + k, qx, qy, qz, best, bi);
                        }
                    }
                }
                const float b = (float)k - kRingMargin;
                if (b > 0.0f) {
                    const float rb = b * a.g.cell;
                    const float rb2 = rb * rb;
                    if (best <= rb2 || rb2 >= a.max_d2) break;
                }
                if (cx - k <= 0 && cx + k >= nx - 1 && cy - k <= 0 && cy + k >= ny - 1 && cz - k <= 0 && cz + k >= nz - 1) break;
            }
        }
        const bool within = finite && best < INFINITY && best <= a.max_d2;
        const float out_d2 = finite ? (within ? best : INFINITY) : NAN;
        if (a.dist2) a.dist2[qi] = out_d2;
        if (a.index) a.index[qi] = within ? bi : -1;
        if (finite) v[FS_NN_SUM_FINITE] = 1.0;
        if (within) {
            v[FS_NN_SUM_WITHIN] = 1.0;
            v[FS_NN_SUM_DIST] = sqrt((double)best);
#pragma unroll
            for (int t = 0; t < FS_NN_MAX_THRESHOLDS; ++t)
                if (t < a.n_tau && best <= a.tau2[t]) v[FS_NN_SUM_TAU + t] = 1.0;
        }
    }
    if (a.rows) {                                                                       // (uniform over the launch)
        block_sum_waves<kNnF>(v, s_red);
        if (threadIdx.x == 0)
#pragma unroll
            for (int f = 0; f < kNnF; ++f) a.rows[(size_t)blockIdx.x * kNnF + f] = v[f];
    }
}

bool nn_grid_ok(float lx, float ly, float lz, float cell, int nx, int ny, int nz)
{
    if (!host_finite(lx) || !host_finite(ly) || !host_finite(lz)) return false;
    if (!(cell >= 1e-30f && cell <= 1e15f)) return false;                               // (NaN fails)
    if (nx < 1 || ny < 1 || nz < 1 || nx > FS_NN_MAX_SIDE || ny > FS_NN_MAX_SIDE || nz > FS_NN_MAX_SIDE) return false;
    return (long long)nx * ny * nz <= FS_NN_MAX_CELLS;
}

NnGrid nn_grid(float lx, float ly, float lz, float cell, int nx, int ny, int nz)
{
    NnGrid g;
    g.lo[0] = lx; g.lo[1] = ly; g.lo[2] = lz;
    g.cell = cell;
    g.inv_cell = 1.0f / cell;
    g.n[0] = nx; g.n[1] = ny; g.n[2] = nz;
    return g;
}

uint32_t nn_blocks(int32_t n) { return (uint32_t)(((long long)n + kSumThreads - 1) / kSumThreads); }

}  // namespace

}  // namespace fs

using namespace fs;

FS_API int fs_geometry_api_version(void) { return FS_GEOMETRY_API_VERSION; }

FS_API int fs_nn_grid_keys(int32_t N, const float* points, float lo_x, float lo_y, float lo_z, float cell, int32_t n_x, int32_t n_y,
                           int32_t n_z, int32_t* keys, void* stream_)
{
    if (N < 0 || !nn_grid_ok(lo_x, lo_y, lo_z, cell, n_x, n_y, n_z)) return FS_ERR_INVALID_ARG;
    if (N > 0 && (!points || !keys)) return FS_ERR_INVALID_ARG;
    if (N == 0) return FS_OK;
    hipLaunchKernelGGL(nn_keys_kernel, dim3(nn_blocks(N)), dim3(kSumThreads), 0, (hipStream_t)stream_, N, points,
                       nn_grid(lo_x, lo_y, lo_z, cell, n_x, n_y, n_z), keys);
    FS_CHECK_LAUNCH("nn_grid_keys");
    return FS_OK;
}

FS_API int fs_nn_grid_gather(int32_t N, const float* points, const int64_t* order, void* records, void* stream_)
{
    if (N < 0) return FS_ERR_INVALID_ARG;
    if (N > 0 && (!points || !order || !records)) return FS_ERR_INVALID_ARG;
    if ((uintptr_t)records & 15) return FS_ERR_INVALID_ARG;
    if (N == 0) return FS_OK;
    hipLaunchKernelGGL(nn_gather_kernel, dim3(nn_blocks(N)), dim3(kSumThreads), 0, (hipStream_t)stream_, N, points,
                       (const long long*)order, (float4*)records);
    FS_CHECK_LAUNCH("nn_grid_gather");
    return FS_OK;
}

FS_API size_t fs_nn_query_scratch_bytes(int32_t Nq)
{
    return Nq <= 0 ? 0 : (size_t)nn_blocks(Nq) * kNnF * sizeof(double);
}

FS_API int fs_nn_query(int32_t Nq, const float* query, const int64_t* query_order, int32_t N_records, const void* records,
                       const int32_t* cell_start, float lo_x, float lo_y, float lo_z, float cell, int32_t n_x, int32_t n_y, int32_t n_z,
                       float max_dist2, int32_t n_tau, const float* tau2, float* dist2, int32_t* index, double* sums, void* scratch,
                       void* stream_)
{
    if (Nq < 0 || N_records < 0 || !nn_grid_ok(lo_x, lo_y, lo_z, cell, n_x, n_y, n_z)) return FS_ERR_INVALID_ARG;
    if (Nq > 0 && (!query || !cell_start)) return FS_ERR_INVALID_ARG;
    if ((N_records > 0 && !records) || ((uintptr_t)records & 15)) return FS_ERR_INVALID_ARG;
    if (!(max_dist2 >= 0.0f)) return FS_ERR_INVALID_ARG;
    if (n_tau < 0 || n_tau > FS_NN_MAX_THRESHOLDS || (n_tau > 0 && !tau2)) return FS_ERR_INVALID_ARG;
    for (int t = 0; t < n_tau; ++t)
        if (tau2[t] != tau2[t]) return FS_ERR_INVALID_ARG;
    if (sums && (!scratch || ((uintptr_t)scratch & 7) || ((uintptr_t)sums & 7))) return FS_ERR_INVALID_ARG;
    if (Nq == 0) return FS_OK;

    NnQueryArgs a;
    a.query = query; a.order = (const long long*)query_order; a.rec = (const float4*)records; a.start = cell_start;
    a.dist2 = dist2; a.index = index; a.rows = sums ? (double*)scratch : nullptr;
    a.g = nn_grid(lo_x, lo_y, lo_z, cell, n_x, n_y, n_z);
    a.max_d2 = max_dist2;
    for (int t = 0; t < FS_NN_MAX_THRESHOLDS; ++t) a.tau2[t] = t < n_tau ? tau2[t] : 0.0f;
    a.Nq = Nq; a.Nrec = N_records; a.n_tau = n_tau;
    hipStream_t st = (hipStream_t)stream_;
    const uint32_t blocks = nn_blocks(Nq);
    hipLaunchKernelGGL(nn_query_kernel, dim3(blocks), dim3(kSumThreads), 0, st, a);
    FS_CHECK_LAUNCH("nn_query");
    if (sums) {
        RowOuts<kNnF> outs;
        for (int f = 0; f < kNnF; ++f) {
            outs.out[f] = sums + f;
            outs.scale[f] = 1.0;
        }
        outs.stride = 0;
        hipLaunchKernelGGL((finalize_rows_kernel<kNnF, BlockSum::kWaves, false>), dim3(1), dim3(kSumThreads), 0, st, (int)blocks, 1,
                           (const double*)scratch, outs);
        FS_CHECK_LAUNCH("nn_query_finalize");
    }
    return FS_OK;
}
