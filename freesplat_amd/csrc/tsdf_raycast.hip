// tsdf_raycast.hip -- ray casting of a TSDF volume into depth, normal and colour maps (include/freesplat_ext_raycast.h;
// freesplat_amd.tsdf.TSDFVolume.raycast).
//
//   ONE launch for the V views of a call.  A workgroup of 256 threads owns 16 x 16 pixels of one view, a wavefront an 8 x 8 tile of
//   them: the rays of a wavefront are neighbours, so their samples share cells and their gathers share cache lines.  A thread
//   marches one ray.  A sample is sixteen gathers (eight corner weights, eight corner values) whose addresses depend only on the
//   sample position: all sixteen are issued before the first is consumed, so a march step is one memory round trip.  Lanes
//   outside the image and dead rays take no part and form no address; the colour planes are read only at a valid hit.  No LDS,
//   no atomics, no workgroup waits on another.
//
//   What keeps a bad input from becoming a hang or a fault: the march loop's counter is an integer bounded by max_steps
//   (<= 2^20, checked on the host) and the refinement's by refine (<= 32); a cell index is clamped to [0, n - 2] ON THE FLOATS
//   (NaN gives 0) before it becomes an integer, and no launch is made for a volume with a dimension of 1, so every gather
//   lies inside the planes whatever the cameras hold.
//
// Numerics: fp32, every operation rounded on its own (-ffp-contract=off), divisions and square roots correctly rounded.
#include "fs_common.h"

#include <math.h>

#include "../../include/freesplat_ext_raycast.h"

namespace fs {

namespace {

constexpr int kTileRc = FS_RAYCAST_TILE;
constexpr int kThreadsRc = kTileRc * kTileRc;
static_assert(kThreadsRc == 4 * kWave, "a workgroup is 2 x 2 wavefront tiles of 8 x 8 pixels");
constexpr long long kMaxIndex = 0x7FFFFFFFll;

struct RaycastArgs {
    const float* tsdf;
    const float* weight;
    const float* color;
    const float* c2w;
    const float* intr;
    float* depth;
    float* normals;
    float* out_color;
    int32_t* steps;
    float ox, oy, oz, vs, trunc, min_depth, max_depth, min_weight, step_min, relax;
    int X, Y, Z, V, H, W, refine, max_steps;
    uint32_t tiles_x, tiles_per_view;
};

// fminf / fmaxf with the choice they leave open fixed (the header): a NaN is dropped, of a +0 / -0 pair the second is returned
__device__ __forceinline__ float min2(float a, float b) { return (a < b || b != b) ? a : b; }
__device__ __forceinline__ float max2(float a, float b) { return (a > b || b != b) ? a : b; }

__device__ __forceinline__ float lerp(float a, float b, float t) { return a + t * (b - a); }

// the cell of a grid coordinate along one axis (nm2 = (float)(n - 2) >= 0): index in [0, n - 2] and the offset inside the cell
__device__ __forceinline__ float cell_of(float g, float nm2, int& i)
{
    const float fl = floorf(g);
    float fi = fl > 0.0f ? fl : 0.0f;            // (NaN: 0)
    fi = fi < nm2 ? fi : nm2;
    i = (int)fi;
    return g - fi;
}

__device__ __forceinline__ void load8(const float* __restrict__ p, long long sy, long long sz, float (&c)[8])
{
    c[0] = p[0];       c[1] = p[1];           c[2] = p[sy];      c[3] = p[sy + 1];
    c[4] = p[sz];      c[5] = p[sz + 1];      c[6] = p[sz + sy]; c[7] = p[sz + sy + 1];
}

__device__ __forceinline__ float trilerp(const float (&c)[8], float tx, float ty, float tz)
{
    const float c00 = lerp(c[0], c[1], tx), c01 = lerp(c[2], c[3], tx), c10 = lerp(c[4], c[5], tx), c11 = lerp(c[6], c[7], tx);
    return lerp(lerp(c00, c01, ty), lerp(c10, c11, ty), tz);
}

struct Ray {
    float o[3], d[3];
};

struct Sample {
    long long cell;      // linear index of corner 0
    float t[3];
    float f;
    bool observed;
};

// step 4 of the header; `corners` receives the eight values
__device__ __forceinline__ Sample sample_at(const RaycastArgs& a, const Ray& r, float s, float (&corners)[8])
{
    Sample out;
    int i, j, k;
    out.t[0] = cell_of(r.o[0] + s * r.d[0], (float)(a.X - 2), i);
    out.t[1] = cell_of(r.o[1] + s * r.d[1], (float)(a.Y - 2), j);
    out.t[2] = cell_of(r.o[2] + s * r.d[2], (float)(a.Z - 2), k);
    const long long sy = a.X, sz = (long long)a.X * a.Y;
    out.cell = ((long long)k * a.Y + j) * a.X + i;
    float w[8];
    load8(a.weight + out.cell, sy, sz, w);       // sixteen independent gathers, issued together
    load8(a.tsdf + out.cell, sy, sz, corners);
    bool obs = true;
#pragma unroll
    for (int q = 0; q < 8; ++q) obs = obs && (w[q] >= a.min_weight);
    out.observed = obs;
    out.f = trilerp(corners, out.t[0], out.t[1], out.t[2]);
    return out;
}

__global__ __launch_bounds__(kThreadsRc) void tsdf_raycast_kernel(const RaycastArgs a)
{
    const uint32_t b = blockIdx.x;
    const uint32_t v = b / a.tiles_per_view, tile = b % a.tiles_per_view;
    const uint32_t tyi = tile / a.tiles_x, txi = tile % a.tiles_x;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int px = (int)txi * kTileRc + (wave & 1) * 8 + (lane & 7);
    const int py = (int)tyi * kTileRc + (wave >> 1) * 8 + (lane >> 3);
    if (px >= a.W || py >= a.H) return;

    const float* __restrict__ m = a.c2w + 12ll * v;
    const float* __restrict__ kk = a.intr + 4ll * v;
    const float dx = ((float)px - kk[2]) / kk[0], dy = ((float)py - kk[3]) / kk[1];
    const float org[3] = {a.ox, a.oy, a.oz};
    const int n[3] = {a.X, a.Y, a.Z};
    Ray r;
    float s0 = a.min_depth, s1 = a.max_depth;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        r.o[c] = (m[4 * c + 3] - org[c]) / a.vs;
        r.d[c] = ((m[4 * c] * dx + m[4 * c + 1] * dy) + m[4 * c + 2]) / a.vs;
        const float lo = (0.0f - r.o[c]) / r.d[c], hi = ((float)(n[c] - 1) - r.o[c]) / r.d[c];
        s0 = max2(s0, min2(lo, hi));
        s1 = min2(s1, max2(lo, hi));
    }
    const float L = sqrtf((r.d[0] * r.d[0] + r.d[1] * r.d[1]) + r.d[2] * r.d[2]);
    const float tv = a.trunc / a.vs;
    const float step_unobserved = a.relax * tv;

    const long long HW = (long long)a.H * a.W;
    const long long pix = (long long)py * a.W + px;
    float depth = 0.0f, nrm[3] = {NAN, NAN, NAN}, col[3] = {0.0f, 0.0f, 0.0f};
    int steps = 0;

    if (s0 <= s1) {                                                   // (the host launches nothing for a volume without a cell)
        float corners[8];
        float sa = 0.0f, fa = 0.0f, sb = 0.0f, fb = 0.0f;
        bool prev_observed = false, hit = false;
        float s = s0;
        for (int it = 0; it < a.max_steps; ++it) {
            const Sample q = sample_at(a, r, s, corners);
            ++steps;
            if (prev_observed && q.observed && !(fa < 0.0f) && q.f < 0.0f) {
                sb = s; fb = q.f;
                hit = true;
                break;
            }
            sa = s; fa = q.f; prev_observed = q.observed;
            const float step = q.observed ? fmaxf(a.step_min, a.relax * (fabsf(q.f) * tv)) : step_unobserved;
            s = s + step / L;
            if (!(s <= s1)) break;
        }
        if (hit) {
            for (int it = 0; it < a.refine; ++it) {
                const float sm = sa + (fa / (fa - fb)) * (sb - sa);
                const Sample q = sample_at(a, r, sm, corners);
                if (q.observed) {
                    if (q.f < 0.0f) { sb = sm; fb = q.f; }
                    else { sa = sm; fa = q.f; }
                }
            }
            depth = sa + (fa / (fa - fb)) * (sb - sa);
            const Sample q = sample_at(a, r, depth, corners);
            const float* c = corners;
            const float tx = q.t[0], ty = q.t[1], tz = q.t[2];
            const float G[3] = {
                lerp(lerp(c[1] - c[0], c[3] - c[2], ty), lerp(c[5] - c[4], c[7] - c[6], ty), tz),
                lerp(lerp(c[2] - c[0], c[3] - c[1], tx), lerp(c[6] - c[4], c[7] - c[5], tx), tz),
                lerp(lerp(c[4] - c[0], c[5] - c[1], tx), lerp(c[6] - c[2], c[7] - c[3], tx), ty)};
            float mm[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) mm[j] = -((m[j] * G[0] + m[4 + j] * G[1]) + m[8 + j] * G[2]);
            const float len = sqrtf((mm[0] * mm[0] + mm[1] * mm[1]) + mm[2] * mm[2]);
            if (q.observed && len > 0.0f && len < INFINITY) {
#pragma unroll
                for (int j = 0; j < 3; ++j) nrm[j] = mm[j] / len;
                if (a.out_color) {
                    const long long P = (long long)a.X * a.Y * a.Z, sy = a.X, sz = (long long)a.X * a.Y;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        float cc[8];
                        load8(a.color + ch * P + q.cell, sy, sz, cc);
                        col[ch] = trilerp(cc, tx, ty, tz);
                    }
                }
            }
        }
    }

    const long long o1 = (long long)v * HW + pix, o3 = (long long)v * 3 * HW + pix;
    a.depth[o1] = depth;
    if (a.steps) a.steps[o1] = steps;
    if (a.normals) {
#pragma unroll
        for (int j = 0; j < 3; ++j) a.normals[o3 + j * HW] = nrm[j];
    }
    if (a.out_color) {
#pragma unroll
        for (int j = 0; j < 3; ++j) a.out_color[o3 + j * HW] = col[j];
    }
}

// what a volume without a cell gives: no ray is alive, nothing of the volume is read
__global__ __launch_bounds__(kThreadsRc) void tsdf_raycast_dead_kernel(long long n1, float* __restrict__ depth, float* __restrict__ normals,
                                                                      float* __restrict__ out_color, int32_t* __restrict__ steps)
{
    const long long i = (long long)blockIdx.x * kThreadsRc + threadIdx.x;
    if (i < n1) {
        depth[i] = 0.0f;
        if (steps) steps[i] = 0;
    }
    if (i < 3 * n1) {
        if (normals) normals[i] = NAN;
        if (out_color) out_color[i] = 0.0f;
    }
}

}  // namespace

}  // namespace fs

using namespace fs;

FS_API int fs_raycast_api_version(void) { return FS_RAYCAST_API_VERSION; }

FS_API int fs_tsdf_raycast(int32_t X, int32_t Y, int32_t Z, float ox, float oy, float oz, float voxel_size, float trunc,
                           const float* tsdf, const float* weight, const float* color, int32_t V, int32_t H, int32_t W,
                           const float* cam_to_world, const float* intrinsics, float min_depth, float max_depth, float min_weight,
                           float step_min, float relax, int32_t refine, int32_t max_steps, float* depth, float* normals,
                           float* out_color, int32_t* steps, void* stream_)
{
    if (X <= 0 || Y <= 0 || Z <= 0 || V <= 0 || H <= 0 || W <= 0) return FS_ERR_INVALID_ARG;
    if (!tsdf || !weight || !cam_to_world || !intrinsics || !depth) return FS_ERR_INVALID_ARG;
    if (out_color && !color) return FS_ERR_INVALID_ARG;
    if (!host_finite(ox) || !host_finite(oy) || !host_finite(oz)) return FS_ERR_INVALID_ARG;
    if (!host_pos_finite(voxel_size) || !host_pos_finite(trunc) || !host_pos_finite(step_min) || !host_pos_finite(relax)) return FS_ERR_INVALID_ARG;
    if (!(min_depth >= 0.0f) || max_depth != max_depth || !(min_weight > 0.0f)) return FS_ERR_INVALID_ARG;
    if (refine < 0 || refine > FS_RAYCAST_MAX_REFINE || max_steps < 1 || max_steps > FS_RAYCAST_MAX_STEPS) return FS_ERR_INVALID_ARG;
    if ((long long)X * Y > kMaxIndex || (long long)X * Y * Z > kMaxIndex || (long long)H * W > kMaxIndex) return FS_ERR_UNSUPPORTED;
    const long long tiles_x = (W + kTileRc - 1) / kTileRc, tiles_y = (H + kTileRc - 1) / kTileRc;
    const long long blocks = tiles_x * tiles_y * V;                                     // (< 2^62)
    const long long n1 = (long long)V * H * W;
    if (blocks > kMaxIndex || (3 * n1 + kThreadsRc - 1) / kThreadsRc > kMaxIndex) return FS_ERR_UNSUPPORTED;

    hipStream_t st = (hipStream_t)stream_;
    if (X < 2 || Y < 2 || Z < 2) {
        const long long nb = (3 * n1 + kThreadsRc - 1) / kThreadsRc;
        hipLaunchKernelGGL(tsdf_raycast_dead_kernel, dim3((uint32_t)nb), dim3(kThreadsRc), 0, st, n1, depth, normals, out_color, steps);
        FS_CHECK_LAUNCH("tsdf_raycast");
        return FS_OK;
    }
    RaycastArgs a;
    a.tsdf = tsdf; a.weight = weight; a.color = color; a.c2w = cam_to_world; a.intr = intrinsics;
    a.depth = depth; a.normals = normals; a.out_color = out_color; a.steps = steps;
    a.ox = ox; a.oy = oy; a.oz = oz; a.vs = voxel_size; a.trunc = trunc;
    a.min_depth = min_depth; a.max_depth = max_depth; a.min_weight = min_weight; a.step_min = step_min; a.relax = relax;
    a.X = X; a.Y = Y; a.Z = Z; a.V = V; a.H = H; a.W = W; a.refine = refine; a.max_steps = max_steps;
    a.tiles_x = (uint32_t)tiles_x;
    a.tiles_per_view = (uint32_t)(tiles_x * tiles_y);
    hipLaunchKernelGGL(tsdf_raycast_kernel, dim3((uint32_t)blocks), dim3(kThreadsRc), 0, st, a);
    FS_CHECK_LAUNCH("tsdf_raycast");
    return FS_OK;
}
