// tsdf.hip -- volumetric TSDF fusion of depth maps and marching-tetrahedra extraction (include/freesplat_amd_tsdf.h;
// freesplat_amd.tsdf.TSDFVolume.integrate / extract_mesh).
//
//   integrate   ONE launch for the V <= 64 views of a call.  A workgroup of 256 threads owns a brick of 32 x 8 x 4 grid points, a
//               thread four consecutive x of it; a wavefront is one z-slice of the brick (32 x 8), so a view's gathers of a
//               wavefront fall into one small patch of the depth map.  The running (tsdf, weight, colour) of the four points
//               stay in registers over the views: the volume is read once (and only where a view updates a point of the thread)
//               and written once (only the updated points).  A view runs in phases -- project the four points, gather depth,
//               decide, gather the image, update -- so that a view costs two dependent memory round trips, not eight.
//               16-byte accesses through fs::load4 / fs::store4 where the four
//               points lie inside the row, start on a 16-byte boundary and (for the store) were all updated, dword accesses
//               otherwise.  Which views can touch the brick is decided first, one lane per view, as a 64-bit ballot that every
//               wavefront forms for itself (no LDS, no barrier): view_may_touch below, result-neutral by monotonicity.
//   mesh plan   count: a thread classifies one cube, a workgroup FS_TSDF_MESH_RUN = 256 consecutive cubes; one workgroup scans the
//               block counts into 64-bit offsets (fs_scan.h's slice_scan: any number of blocks is covered).
//   mesh emit   a thread derives its cube's cases again, the workgroup scans its 256 counts (block_excl_scan), the thread
//               writes its triangles.
//
// Numerics: fp32, every operation rounded on its own (-ffp-contract=off), divisions correctly rounded.  No float atomics, no
// workgroup waits on another: the same bits on every run and stream.
#include "fs_common.h"

#include <math.h>

#include "../../include/freesplat_amd_tsdf.h"
#include "fs_reduce.h"
#include "fs_scan.h"

namespace fs {

namespace {

constexpr int kBX = FS_TSDF_BRICK_X, kBY = FS_TSDF_BRICK_Y, kBZ = FS_TSDF_BRICK_Z;
constexpr int kThreads = kSumThreads;
static_assert(kBX / 4 * kBY * kBZ == kThreads && kBX / 4 * kBY == kWave, "a wavefront is one z-slice of the brick");
static_assert(FS_TSDF_MAX_VIEWS == kWave, "the view list of a brick is one ballot");
constexpr int kRun = FS_TSDF_MESH_RUN;
static_assert(kRun == kThreads, "a thread of the extraction owns one cube");
constexpr long long kMaxPoints = 0x7FFFFFFFll;

// ------------------------------------------------------------------------------------------------------------ integrate

struct IntegrateArgs {
    float* tsdf;
    float* weight;
    float* color;
    const float* w2c;
    const float* intr;
    const float* depth;
    const float* alpha;
    const float* image;
    float ox, oy, oz, vs, trunc, max_weight, near, min_depth, max_depth, alpha_min, alpha_floor;
    int X, Y, Z, V, H, W;
    uint32_t nbx, nby;
    int skip;
};

__device__ __forceinline__ float grid_coord(float o, float vs, int i) { return o + vs * (float)i; }

// row c of [R | t] applied to a point, in the header's association
__device__ __forceinline__ float cam_row(const float* __restrict__ m, float x, float y, float z)
{
    return ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
}

__device__ __forceinline__ float project(float f, float c, float p, float pz) { return f * (p / pz) + c; }

__device__ __forceinline__ bool finite(float x) { return fabsf(x) < INFINITY; }

// Can view v update a grid point of the box [bx] x [by] x [bz] (its first and last grid coordinates)?  false only when every
// point of the box fails `p_z > near` or the pixel range test.  Each of cam_row's and project's operations is a correctly
// rounded product, sum or quotient, hence monotone in each operand (the quotient for p_z > 0); the grid coordinates are
// monotone in the index.  So a point's p_c lies between the least and the greatest of the eight corners' p_c, its p / p_z
// between the extremes of the four quotients of those bounds, and rint(u) between the rint of the bounds of u.  Anything not
// finite: no verdict, the view is walked.
__device__ bool view_may_touch(const IntegrateArgs& a, int v, const float (&bx)[2], const float (&by)[2], const float (&bz)[2])
{
    const float* m = a.w2c + 12 * v;
    const float* k = a.intr + 4 * v;
    float lo[3], hi[3];
    bool fin = true;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        lo[c] = INFINITY;
        hi[c] = -INFINITY;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float p = cam_row(m + 4 * c, bx[q & 1], by[(q >> 1) & 1], bz[q >> 2]);
            fin = fin && finite(p);
            lo[c] = fminf(lo[c], p);
            hi[c] = fmaxf(hi[c], p);
        }
    }
    if (!fin) return true;
    if (!(hi[2] > a.near)) return false;
    if (!(lo[2] > 0.0f)) return true;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float q0 = lo[c] / lo[2], q1 = lo[c] / hi[2], q2 = hi[c] / lo[2], q3 = hi[c] / hi[2];
        const float qlo = fminf(fminf(q0, q1), fminf(q2, q3)), qhi = fmaxf(fmaxf(q0, q1), fmaxf(q2, q3));
        const float u0 = k[c] * qlo + k[2 + c], u1 = k[c] * qhi + k[2 + c];
        if (!(finite(q0) && finite(q1) && finite(q2) && finite(q3) && finite(u0) && finite(u1))) return true;
        const float n = (float)(c == 0 ? a.W : a.H);
        if (rintf(fmaxf(u0, u1)) < 0.0f || rintf(fminf(u0, u1)) >= n) return false;
    }
    return true;
}

template <bool COLOR, bool ALPHA>
__global__ __launch_bounds__(kThreads) void tsdf_integrate_kernel(const IntegrateArgs a)
{
    const uint32_t b = blockIdx.x;
    const uint32_t bxi = b % a.nbx, rest = b / a.nbx, byi = rest % a.nby, bzi = rest / a.nby;
    const int t = threadIdx.x;

    // the views of this brick, in order (every wavefront forms the same word)
    unsigned long long views;
    {
        const int lane = t & (kWave - 1);
        bool keep = lane < a.V;
        if (keep && a.skip) {
            const int i0 = (int)bxi * kBX, j0 = (int)byi * kBY, k0 = (int)bzi * kBZ;
            const float bx[2] = {grid_coord(a.ox, a.vs, i0), grid_coord(a.ox, a.vs, min(i0 + kBX, a.X) - 1)};
            const float by[2] = {grid_coord(a.oy, a.vs, j0), grid_coord(a.oy, a.vs, min(j0 + kBY, a.Y) - 1)};
            const float bz[2] = {grid_coord(a.oz, a.vs, k0), grid_coord(a.oz, a.vs, min(k0 + kBZ, a.Z) - 1)};
            keep = view_may_touch(a, lane, bx, by, bz);
        }
        views = __ballot(keep);
    }

    const int i0 = (int)bxi * kBX + (t & 7) * 4, j = (int)byi * kBY + ((t >> 3) & 7), k = (int)bzi * kBZ + (t >> 6);
    if (i0 >= a.X || j >= a.Y || k >= a.Z) return;
    const int n = min(4, a.X - i0);
    const long long row = ((long long)k * a.Y + j) * a.X;
    const long long p0 = row + i0, row_end = row + a.X;
    const long long P = (long long)a.X * a.Y * a.Z;
    const size_t HW = (size_t)a.H * a.W;

    float x[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = grid_coord(a.ox, a.vs, i0 + q);
    const float y = grid_coord(a.oy, a.vs, j), z = grid_coord(a.oz, a.vs, k);

    Px4 f, w, col[3];
    bool loaded = false;
    uint32_t touched = 0;
    const float fW = (float)a.W, fH = (float)a.H;

    // A view in phases, so that the four points' gathers are in flight together (two dependent memory round trips per view,
    // not eight): project all four, gather depth (and alpha), decide, gather the image, update.  A point that is out reads
    // pixel 0 of the map -- a harmless read whose value is dropped; the arithmetic and its order are those of the header.
    while (views) {
        const int v = __builtin_ctzll(views);
        views &= views - 1;
        const float* m = a.w2c + 12 * v;
        const float* kk = a.intr + 4 * v;
        const float* dm = a.depth + (size_t)v * HW;
        float pz[4];
        size_t pix[4];
        uint32_t ok = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            pz[q] = cam_row(m + 8, x[q], y, z);
            const float px = cam_row(m, x[q], y, z), py = cam_row(m + 4, x[q], y, z);
            const float fx = rintf(project(kk[0], kk[2], px, pz[q])), fy = rintf(project(kk[1], kk[3], py, pz[q]));
            const bool in = q < n && pz[q] > a.near && fx >= 0.0f && fx < fW && fy >= 0.0f && fy < fH;
            pix[q] = in ? (size_t)(int)fy * a.W + (size_t)(int)fx : (size_t)0;
            ok |= (in ? 1u : 0u) << q;
        }
        if (!ok) continue;
        float d[4], s[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) d[q] = dm[pix[q]];
        if constexpr (ALPHA) {
            float al[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) al[q] = a.alpha[(size_t)v * HW + pix[q]];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (al[q] < a.alpha_min) ok &= ~(1u << q);
                d[q] = expected_depth<float>(d[q], al[q], true, a.alpha_floor);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float sdf = d[q] - pz[q];
            if (!valid_depth(d[q], a.min_depth, a.max_depth) || sdf < -a.trunc) ok &= ~(1u << q);
            s[q] = fminf(1.0f, sdf / a.trunc);
        }
        if (!ok) continue;
        float c[3][4];
        if constexpr (COLOR) {
            const float* im = a.image + (size_t)v * 3 * HW;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int q = 0; q < 4; ++q) c[ch][q] = im[ch * HW + pix[q]];
        }
        if (!loaded) {
            loaded = true;
            f = load4(a.tsdf, p0, row_end, aligned16(a.tsdf + p0));
            w = load4(a.weight, p0, row_end, aligned16(a.weight + p0));
            if constexpr (COLOR) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) col[ch] = load4(a.color + ch * P, p0, row_end, aligned16(a.color + ch * P + p0));
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!((ok >> q) & 1u)) continue;
            const float W0 = w.v[q], W1 = W0 + 1.0f;
            f.v[q] = (f.v[q] * W0 + s[q]) / W1;
            if constexpr (COLOR) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) col[ch].v[q] = (col[ch].v[q] * W0 + c[ch][q]) / W1;
            }
            w.v[q] = fminf(W1, a.max_weight);
        }
        touched |= ok;
    }
    if (!touched) return;
    if (touched == 0xFu) {                                   // (n == 4) the whole group: 16-byte stores where the base allows
        store4(a.tsdf, p0, row_end, aligned16(a.tsdf + p0), f);
        store4(a.weight, p0, row_end, aligned16(a.weight + p0), w);
        if constexpr (COLOR) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) store4(a.color + ch * P, p0, row_end, aligned16(a.color + ch * P + p0), col[ch]);
        }
    } else {                                                 // a grid point no view updated is not written
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!((touched >> q) & 1u)) continue;
            a.tsdf[p0 + q] = f.v[q];
            a.weight[p0 + q] = w.v[q];
            if constexpr (COLOR) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) a.color[ch * P + p0 + q] = col[ch].v[q];
            }
        }
    }
}

// ----------------------------------------------------------------------------------------------------------------- mesh

// (tet, case) -> number of triangles, then two triangles of three edge codes (A << 3) | B, A < B cube corners: the table of
// include/freesplat_amd_tsdf.h, generated once from its geometric definition (tests/tsdf_ref.py mt_table regenerates it and
// tests/test_tsdf_host.py compares all 96 entries)
constexpr uint8_t kTableInit[6][16][7] = {
    {{0,0,0,0,0,0,0}, {1,1,3,7,0,0,0}, {1,1,15,11,0,0,0}, {2,3,7,15,3,15,11}, {1,3,11,31,0,0,0}, {2,1,31,7,1,11,31}, {2,1,15,31,1,31,3}, {1,7,15,31,0,0,0}, {1,7,31,15,0,0,0}, {2,1,3,31,1,31,15}, {2,1,31,11,1,7,31}, {1,3,31,11,0,0,0}, {2,3,11,15,3,15,7}, {1,1,11,15,0,0,0}, {1,1,7,3,0,0,0}, {0,0,0,0,0,0,0}},
    {{0,0,0,0,0,0,0}, {1,1,7,5,0,0,0}, {1,1,13,15,0,0,0}, {2,5,15,7,5,13,15}, {1,5,47,13,0,0,0}, {2,1,7,47,1,47,13}, {2,1,47,15,1,5,47}, {1,7,47,15,0,0,0}, {1,7,15,47,0,0,0}, {2,1,47,5,1,15,47}, {2,1,13,47,1,47,7}, {1,5,13,47,0,0,0}, {2,5,15,13,5,7,15}, {1,1,15,13,0,0,0}, {1,1,5,7,0,0,0}, {0,0,0,0,0,0,0}},
    {{0,0,0,0,0,0,0}, {1,2,7,3,0,0,0}, {1,2,19,23,0,0,0}, {2,3,23,7,3,19,23}, {1,3,31,19,0,0,0}, {2,2,7,31,2,31,19}, {2,2,31,23,2,3,31}, {1,7,31,23,0,0,0}, {1,7,23,31,0,0,0}, {2,2,31,3,2,23,31}, {2,2,19,31,2,31,7}, {1,3,19,31,0,0,0}, {2,3,23,19,3,7,23}, {1,2,23,19,0,0,0}, {1,2,3,7,0,0,0}, {0,0,0,0,0,0,0}},
    {{0,0,0,0,0,0,0}, {1,2,6,7,0,0,0}, {1,2,23,22,0,0,0}, {2,6,7,23,6,23,22}, {1,6,22,55,0,0,0}, {2,2,55,7,2,22,55}, {2,2,23,55,2,55,6}, {1,7,23,55,0,0,0}, {1,7,55,23,0,0,0}, {2,2,6,55,2,55,23}, {2,2,55,22,2,7,55}, {1,6,55,22,0,0,0}, {2,6,22,23,6,23,7}, {1,2,22,23,0,0,0}, {1,2,7,6,0,0,0}, {0,0,0,0,0,0,0}},
    {{0,0,0,0,0,0,0}, {1,4,5,7,0,0,0}, {1,4,39,37,0,0,0}, {2,5,7,39,5,39,37}, {1,5,37,47,0,0,0}, {2,4,47,7,4,37,47}, {2,4,39,47,4,47,5}, {1,7,39,47,0,0,0}, {1,7,47,39,0,0,0}, {2,4,5,47,4,47,39}, {2,4,47,37,4,7,47}, {1,5,47,37,0,0,0}, {2,5,37,39,5,39,7}, {1,4,37,39,0,0,0}, {1,4,7,5,0,0,0}, {0,0,0,0,0,0,0}},
    {{0,0,0,0,0,0,0}, {1,4,7,6,0,0,0}, {1,4,38,39,0,0,0}, {2,6,39,7,6,38,39}, {1,6,55,38,0,0,0}, {2,4,7,55,4,55,38}, {2,4,55,39,4,6,55}, {1,7,55,39,0,0,0}, {1,7,39,55,0,0,0}, {2,4,55,6,4,39,55}, {2,4,38,55,4,55,7}, {1,6,38,55,0,0,0}, {2,6,39,38,6,7,39}, {1,4,39,38,0,0,0}, {1,4,6,7,0,0,0}, {0,0,0,0,0,0,0}},
};
struct MtTable {
    uint8_t e[6][16][7];
};
constexpr MtTable make_table()
{
    MtTable t{};
    for (int i = 0; i < 6; ++i)
        for (int c = 0; c < 16; ++c)
            for (int k = 0; k < 7; ++k) t.e[i][c][k] = kTableInit[i][c][k];
    return t;
}
constexpr MtTable kHostTable = make_table();
__device__ const MtTable kTable = make_table();

// cube corners of tetrahedron t's vertices 0 .. 3: {c0, c0 + e_a, c0 + e_a + e_b, c7} over the permutations (a, b, .)
__device__ constexpr int kTet[6][4] = {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}};

struct MeshArgs {
    const float* tsdf;
    const float* weight;
    const float* color;
    float ox, oy, oz, vs, min_weight;
    int X, Y, Z;
    long long NC;            // cubes
};

struct Cube {
    int i, j, k;
    long long base;          // linear index of corner 0
};

__device__ __forceinline__ Cube cube_at(const MeshArgs& a, long long c)
{
    Cube q;
    const long long cx = a.X - 1, cy = a.Y - 1;
    const long long r = c / cx;
    q.i = (int)(c - r * cx);
    q.k = (int)(r / cy);
    q.j = (int)(r - (long long)q.k * cy);
    q.base = ((long long)q.k * a.Y + q.j) * a.X + q.i;
    return q;
}

__device__ __forceinline__ long long corner_at(const MeshArgs& a, long long base, int c)
{
    return base + (c & 1) + (long long)((c >> 1) & 1) * a.X + (long long)((c >> 2) & 1) * a.X * a.Y;
}

__device__ __forceinline__ uint32_t triangles_of(uint32_t cs)
{
    const int pc = __popc(cs);
    return pc == 2 ? 2u : (pc == 1 || pc == 3) ? 1u : 0u;
}

// the six 4-bit cases of cube c packed into 24 bits (0: the cube is not live, or not cut) and its number of triangles
__device__ __forceinline__ uint32_t cube_cases(const MeshArgs& a, long long c, Cube& q, uint32_t& count)
{
    count = 0;
    if (c >= a.NC) return 0;
    q = cube_at(a, c);
    bool live = true;
#pragma unroll
    for (int n = 0; n < 8; ++n) live = live && a.weight[corner_at(a, q.base, n)] >= a.min_weight;
    if (!live) return 0;
    uint32_t in = 0;
#pragma unroll
    for (int n = 0; n < 8; ++n) in |= (a.tsdf[corner_at(a, q.base, n)] < 0.0f ? 1u : 0u) << n;
    uint32_t cases = 0;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        uint32_t cs = 0;
#pragma unroll
        for (int m = 0; m < 4; ++m) cs |= ((in >> kTet[t][m]) & 1u) << m;
        cases |= cs << (4 * t);
        count += triangles_of(cs);
    }
    return cases;
}

__global__ __launch_bounds__(kThreads) void tsdf_mesh_count_kernel(const MeshArgs a, uint32_t* __restrict__ block_counts)
{
    __shared__ int s_w[kSumWaves];
    Cube q;
    uint32_t count;
    cube_cases(a, (long long)blockIdx.x * kRun + threadIdx.x, q, count);
    const int tot = wave_sum<int>((int)count);
    if ((threadIdx.x & (kWave - 1)) == 0) s_w[threadIdx.x / kWave] = tot;
    __syncthreads();
    if (threadIdx.x == 0) block_counts[blockIdx.x] = (uint32_t)waves_total<int>(s_w, 1);
}

// One workgroup: exclusive 64-bit scan of the block counts, the sum into *total (fs_scan.h's slice_scan).
__global__ __launch_bounds__(kScanThreads) void tsdf_mesh_scan_kernel(uint32_t nb, const uint32_t* __restrict__ block_counts,
                                                                      unsigned long long* __restrict__ block_offsets,
                                                                      long long* __restrict__ total)
{
    __shared__ unsigned long long part[kScanThreads];
    const unsigned long long sum = slice_scan<unsigned long long>(block_counts, nb, block_offsets, part);
    if (threadIdx.x == kScanThreads - 1) *total = (long long)sum;
}

// one cut vertex: position and (COLOR) colour of edge code e of cube q
template <bool COLOR>
__device__ __forceinline__ void cut_vertex(const MeshArgs& a, const Cube& q, uint32_t e, float* __restrict__ pos, float* __restrict__ rgb)
{
    const int A = (int)(e >> 3), B = (int)(e & 7u);
    const long long g0 = corner_at(a, q.base, A), g1 = corner_at(a, q.base, B);
    const float f0 = a.tsdf[g0], f1 = a.tsdf[g1];
    const float t = f0 / (f0 - f1);
    const float o[3] = {a.ox, a.oy, a.oz};
    const int idx[3] = {q.i, q.j, q.k};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float P0 = grid_coord(o[c], a.vs, idx[c] + ((A >> c) & 1)), P1 = grid_coord(o[c], a.vs, idx[c] + ((B >> c) & 1));
        pos[c] = P0 + t * (P1 - P0);
    }
    if constexpr (COLOR) {
        const long long P = (long long)a.X * a.Y * a.Z;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float c0 = a.color[c * P + g0], c1 = a.color[c * P + g1];
            rgb[c] = c0 + t * (c1 - c0);
        }
    }
}

template <bool COLOR>
__global__ __launch_bounds__(kThreads) void tsdf_mesh_emit_kernel(const MeshArgs a, const unsigned long long* __restrict__ block_offsets,
                                                                  long long T, float* __restrict__ vertices, float* __restrict__ colors)
{
    __shared__ uint32_t s_w[kSumWaves];
    Cube q;
    uint32_t count;
    const uint32_t cases = cube_cases(a, (long long)blockIdx.x * kRun + threadIdx.x, q, count);
    const uint32_t before = block_excl_scan(count, s_w);
    if (count == 0) return;
    long long tri = (long long)block_offsets[blockIdx.x] + before;
    for (int t = 0; t < 6; ++t) {
        const uint32_t cs = (cases >> (4 * t)) & 15u;
        const uint32_t n = triangles_of(cs);
        for (uint32_t k = 0; k < n; ++k, ++tri) {
            if (tri >= T) return;
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                float pos[3], rgb[3];
                cut_vertex<COLOR>(a, q, kTable.e[t][cs][1 + 3 * k + e], pos, rgb);
                float* out = vertices + tri * 9 + e * 3;
                out[0] = pos[0]; out[1] = pos[1]; out[2] = pos[2];
                if constexpr (COLOR) {
                    float* oc = colors + tri * 9 + e * 3;
                    oc[0] = rgb[0]; oc[1] = rgb[1]; oc[2] = rgb[2];
                }
            }
        }
    }
}

// 0: fine; else the status
int check_dims(int32_t X, int32_t Y, int32_t Z)
{
    if (X <= 0 || Y <= 0 || Z <= 0) return FS_ERR_INVALID_ARG;
    if ((long long)X * Y > kMaxPoints || (long long)X * Y * Z > kMaxPoints) return FS_ERR_UNSUPPORTED;
    return FS_OK;
}

long long cubes_of(int32_t X, int32_t Y, int32_t Z) { return (long long)(X - 1) * (Y - 1) * (Z - 1); }
size_t mesh_blocks(long long NC) { return (size_t)((NC + kRun - 1) / kRun); }
size_t counts_bytes(size_t nb) { return align_up((nb ? nb : 1) * sizeof(uint32_t), 256); }

MeshArgs mesh_args(int32_t X, int32_t Y, int32_t Z, const float* tsdf, const float* weight, const float* color, float min_weight)
{
    MeshArgs a;
    a.tsdf = tsdf; a.weight = weight; a.color = color;
    a.ox = a.oy = a.oz = 0.0f; a.vs = 1.0f; a.min_weight = min_weight;
    a.X = X; a.Y = Y; a.Z = Z;
    a.NC = cubes_of(X, Y, Z);
    return a;
}

}  // namespace

}  // namespace fs

using namespace fs;

FS_API int fs_tsdf_api_version(void) { return FS_TSDF_API_VERSION; }

FS_API int fs_tsdf_integrate(int32_t X, int32_t Y, int32_t Z, float ox, float oy, float oz, float voxel_size, float trunc,
                             float max_weight, float* tsdf, float* weight, float* color, int32_t V, int32_t H, int32_t W,
                             const float* world_to_cam, const float* intrinsics, const float* depth, const float* alpha,
                             const float* image, float near, float min_depth, float max_depth, float alpha_min, float alpha_floor,
                             int32_t flags, void* stream_)
{
    if (X <= 0 || Y <= 0 || Z <= 0 || V <= 0 || H <= 0 || W <= 0) return FS_ERR_INVALID_ARG;
    if (!tsdf || !weight || !world_to_cam || !intrinsics || !depth) return FS_ERR_INVALID_ARG;
    if ((color == nullptr) != (image == nullptr)) return FS_ERR_INVALID_ARG;
    if (!host_finite(ox) || !host_finite(oy) || !host_finite(oz)) return FS_ERR_INVALID_ARG;
    if (near != near || min_depth != min_depth || max_depth != max_depth || alpha_min != alpha_min) return FS_ERR_INVALID_ARG;
    if (!host_pos_finite(voxel_size) || !host_pos_finite(trunc) || !host_pos_finite(max_weight) || !host_pos_finite(alpha_floor)) return FS_ERR_INVALID_ARG;
    if (flags & ~FS_TSDF_NO_BRICK_SKIP) return FS_ERR_INVALID_ARG;
    if (V > FS_TSDF_MAX_VIEWS) return FS_ERR_UNSUPPORTED;
    if (check_dims(X, Y, Z) != FS_OK || (long long)H * W > kMaxPoints) return FS_ERR_UNSUPPORTED;

    IntegrateArgs a;
    a.tsdf = tsdf; a.weight = weight; a.color = color;
    a.w2c = world_to_cam; a.intr = intrinsics; a.depth = depth; a.alpha = alpha; a.image = image;
    a.ox = ox; a.oy = oy; a.oz = oz; a.vs = voxel_size; a.trunc = trunc; a.max_weight = max_weight;
    a.near = near; a.min_depth = min_depth; a.max_depth = max_depth; a.alpha_min = alpha_min; a.alpha_floor = alpha_floor;
    a.X = X; a.Y = Y; a.Z = Z; a.V = V; a.H = H; a.W = W;
    a.nbx = (uint32_t)((X + kBX - 1) / kBX);
    a.nby = (uint32_t)((Y + kBY - 1) / kBY);
    a.skip = (flags & FS_TSDF_NO_BRICK_SKIP) ? 0 : 1;
    const long long blocks = (long long)a.nbx * a.nby * ((Z + kBZ - 1) / kBZ);          // <= X * Y * Z
    const dim3 grid((uint32_t)blocks), block(kThreads);
    hipStream_t st = (hipStream_t)stream_;
    if (color) {
        if (alpha) hipLaunchKernelGGL((tsdf_integrate_kernel<true, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((tsdf_integrate_kernel<true, false>), grid, block, 0, st, a);
    } else {
        if (alpha) hipLaunchKernelGGL((tsdf_integrate_kernel<false, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((tsdf_integrate_kernel<false, false>), grid, block, 0, st, a);
    }
    FS_CHECK_LAUNCH("tsdf_integrate");
    return FS_OK;
}

FS_API int fs_tsdf_mt_table(uint8_t* table)
{
    if (!table) return FS_ERR_INVALID_ARG;
    for (int t = 0; t < 6; ++t)
        for (int c = 0; c < 16; ++c)
            for (int k = 0; k < 7; ++k) table[(t * 16 + c) * 7 + k] = kHostTable.e[t][c][k];
    return FS_OK;
}

FS_API size_t fs_tsdf_mesh_scratch_bytes(int32_t X, int32_t Y, int32_t Z)
{
    if (check_dims(X, Y, Z) != FS_OK) return 0;
    const size_t nb = mesh_blocks(cubes_of(X, Y, Z));
    return counts_bytes(nb) + align_up((nb ? nb : 1) * sizeof(unsigned long long), 256);
}

FS_API int fs_tsdf_mesh_plan(int32_t X, int32_t Y, int32_t Z, const float* tsdf, const float* weight, float min_weight,
                             int64_t* total, void* scratch, void* stream_)
{
    if (X <= 0 || Y <= 0 || Z <= 0) return FS_ERR_INVALID_ARG;
    if (!tsdf || !weight || !total || !scratch) return FS_ERR_INVALID_ARG;
    if (!(min_weight > 0.0f)) return FS_ERR_INVALID_ARG;
    if (check_dims(X, Y, Z) != FS_OK) return FS_ERR_UNSUPPORTED;
    const MeshArgs a = mesh_args(X, Y, Z, tsdf, weight, nullptr, min_weight);
    const size_t nb = mesh_blocks(a.NC);
    uint32_t* counts = (uint32_t*)scratch;
    unsigned long long* offsets = (unsigned long long*)((char*)scratch + counts_bytes(nb));
    hipStream_t st = (hipStream_t)stream_;
    if (nb) hipLaunchKernelGGL(tsdf_mesh_count_kernel, dim3((uint32_t)nb), dim3(kThreads), 0, st, a, counts);
    hipLaunchKernelGGL(tsdf_mesh_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, (uint32_t)nb, (const uint32_t*)counts, offsets,
                       (long long*)total);
    FS_CHECK_LAUNCH("tsdf_mesh_plan");
    return FS_OK;
}

FS_API int fs_tsdf_mesh_emit(int32_t X, int32_t Y, int32_t Z, float ox, float oy, float oz, float voxel_size, const float* tsdf,
                             const float* weight, const float* color, float min_weight, const void* scratch, int64_t T,
                             float* vertices, float* colors, void* stream_)
{
    if (X <= 0 || Y <= 0 || Z <= 0 || T < 0) return FS_ERR_INVALID_ARG;
    if (!tsdf || !weight || !scratch) return FS_ERR_INVALID_ARG;
    if ((color == nullptr) != (colors == nullptr) && T > 0) return FS_ERR_INVALID_ARG;
    if (T > 0 && !vertices) return FS_ERR_INVALID_ARG;
    if (!(min_weight > 0.0f) || !host_finite(ox) || !host_finite(oy) || !host_finite(oz) || !host_pos_finite(voxel_size)) return FS_ERR_INVALID_ARG;
    if (check_dims(X, Y, Z) != FS_OK || T > kMaxPoints / 9) return FS_ERR_UNSUPPORTED;
    if (T == 0) return FS_OK;
    MeshArgs a = mesh_args(X, Y, Z, tsdf, weight, color, min_weight);
    a.ox = ox; a.oy = oy; a.oz = oz; a.vs = voxel_size;
    const size_t nb = mesh_blocks(a.NC);
    if (nb == 0) return FS_ERR_INVALID_ARG;                 // a volume without a cube has no triangle
    const unsigned long long* offsets = (const unsigned long long*)((const char*)scratch + counts_bytes(nb));
    hipStream_t st = (hipStream_t)stream_;
    if (color) hipLaunchKernelGGL(tsdf_mesh_emit_kernel<true>, dim3((uint32_t)nb), dim3(kThreads), 0, st, a, offsets, (long long)T, vertices, colors);
    else hipLaunchKernelGGL(tsdf_mesh_emit_kernel<false>, dim3((uint32_t)nb), dim3(kThreads), 0, st, a, offsets, (long long)T, vertices, colors);
    FS_CHECK_LAUNCH("tsdf_mesh_emit");
    return FS_OK;
}
