// mv_depth_loss.hip -- the multi-view depth consistency term and the scale-invariant depth term
// (include/freesplat_amd_mvdepth.h, DESIGN.md "Multi-view depth loss"), forward and backward.
//
// Multi-view term: the sensor depth gt of a pixel of view b is moved into each of the view's K source cameras with the pair's
// twelve floats [A | t] (q = gt A (x, y, 1)^T + t), the source's sensor depth S is read at the nearest pixel, and where the
// point is not occluded there (z' < occlusion S) the PREDICTED depth, moved along the same ray, is compared with S in log space.
//
// One pass over three maps with K dependent gathers.  A workgroup owns kChunk consecutive pixels of ONE view (blockIdx.x =
// view * chunks + chunk), a thread one group of four consecutive pixels; a group starts at a pixel index that is a multiple of
// four, so whether a plane can be accessed with 16-byte loads and stores depends on the plane's base address alone: an aligned
// plane goes through float4, any other plane and the last, partial group go through dword accesses with a bound check.  The
// path changes nothing about a pixel's arithmetic or about the thread that owns it.  The view, the source map and the pair's
// twelve floats are workgroup-uniform (scalar loads); the loop over the K sources is rolled.
//
// Arithmetic: the gather location and the visibility test follow the definition in fp32 (explicit fmaf).  From the predicted
// depth on a pixel is carried in fp64: E = depth / max(alpha, floor), z_p' = E a[2] + t[2] + 1e-8, the ratio z_p' / S, and the
// logarithm as logf of the ratio rounded to fp32 plus the first-order term of what the rounding dropped (log_of()): the fp32
// chain would put its 1e-7 on a residual of a few 1e-2.  These are some ten fp64 operations per pixel and source.
//
// Sums: a thread's pixels in index order in fp64, the block_sum_waves order of fs_reduce.h per workgroup, one row of partials
// per workgroup and source in the caller's scratch, and finalize_rows_kernel with one workgroup per (view, source).  Counts are integers.  The partition depends on (H, W) only.  No float
// atomics, no workgroup waits on another.
//
// Backward: a gather per pixel that recomputes S and the selection from the inputs; every pixel of g_depth / g_alpha is
// written by exactly one thread.  The forward saves nothing.
#include "fs_reduce.h"

#include "../../include/freesplat_amd_mvdepth.h"

namespace fs {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kSumWaves;
constexpr int kVec = 4;                              // pixels of a group: one 16-byte access per plane
constexpr int kChunk = kThreads * kVec;              // pixels per workgroup (freesplat_amd/mv_depth_loss.py CHUNK)
constexpr int kMaxK = FS_MVDEPTH_MAX_SOURCES;
constexpr float kEps = 1e-8f;                        // the projection's epsilon

struct Params {
    float occlusion, min_depth, max_depth, alpha_floor;
};

// log of a positive finite double in the fp32 range: logf of the value rounded to fp32 (its error is relative to the RESULT)
// plus the first-order term of the 6e-8 the rounding dropped (the second-order term is 2e-15).  A value near the ends of the
// fp32 range, where that rounding is coarser, takes the fp64 logarithm.
__device__ __forceinline__ double log_of(double x)
{
    const float q = (float)x;
    if (!(q > 1e-30f && q < 1e30f)) return log(x);
    return (double)logf(q) + (double)((float)(x - (double)q) / q);
}

// a thread's group: the three maps' values, the pixel coordinates and the expected depth of its four pixels
struct Group {
    long long p0;           // first pixel
    bool v0[kVec];          // inside the view and gt valid
    float g[kVec], m[kVec], xf[kVec], yf[kVec];      // gt, max(alpha, floor) (1 without alpha), the pixel's column and row
    float al[kVec];         // alpha (1 without)
    double E[kVec];
};

__device__ __forceinline__ Group load_group(long long p0, long long P, int W, const float* __restrict__ depth,
                                            const float* __restrict__ gt, const float* __restrict__ alpha, const Params& Q)
{
    Group G;
    G.p0 = p0;
    const Px4 d = load4(depth, p0, P, aligned16(depth));
    const Px4 g = load4(gt, p0, P, aligned16(gt));
    Px4 a;
    if (alpha) {
        a = load4(alpha, p0, P, aligned16(alpha));
    } else {
#pragma unroll
        for (int j = 0; j < kVec; ++j) a.v[j] = 1.0f;
    }
    const long long pc = p0 < P ? p0 : 0;
    int y = (int)(pc / W), x = (int)(pc - (long long)y * W);
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
        G.g[j] = g.v[j];
        G.al[j] = a.v[j];
        G.m[j] = alpha ? fmaxf(a.v[j], Q.alpha_floor) : 1.0f;
        G.v0[j] = p0 + j < P && valid_depth(g.v[j], Q.min_depth, Q.max_depth);
        G.E[j] = expected_depth<double>(d.v[j], a.v[j], alpha != nullptr, Q.alpha_floor);
        G.xf[j] = (float)x;
        G.yf[j] = (float)y;
        if (++x == W) {
            x = 0;
            ++y;
        }
    }
    return G;
}

// what a workgroup knows of its pair (view b, source k): all of it wave-uniform
struct Pair {
    const float* src;       // the source map, nullptr: an index out of range, the pair contributes nothing
    float a[9], t[3];       // A row-major, t
};

__device__ __forceinline__ Pair pair_of(long long b, int k, int K, long long Ps, int S_pool, const float* __restrict__ src_depth,
                                        const int* __restrict__ src_index, const float* __restrict__ pairs)
{
    Pair M;
    const long long bk = b * K + k;
    long long map = bk;
    bool on = true;
    if (src_index) {
        map = src_index[bk];
        on = map >= 0 && map < (long long)S_pool;
    }
    M.src = on ? src_depth + (size_t)map * (size_t)Ps : nullptr;         // (an index out of range never forms an address)
    const float* q = pairs + (size_t)bk * 12;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) M.a[r * 3 + c] = q[r * 4 + c];
        M.t[r] = q[r * 4 + 3];
    }
    return M;
}

// Pixel j of the group against the pair: false = not selected.  S: the source's sample, a2 = (A (x, y, 1)^T)[2],
// zp = z_p' (fp64).  The source is read only for a pixel whose gt is valid and whose projection lands inside the map.
__device__ __forceinline__ bool select(const Pair& M, const Group& G, int j, int Hs, int Ws, const Params& Q, float& S, double& a2,
                                       double& zp)
{
    if (!G.v0[j]) return false;
    const float x = G.xf[j], y = G.yf[j], g = G.g[j];
    const float r0 = fmaf(M.a[0], x, fmaf(M.a[1], y, M.a[2]));
    const float r1 = fmaf(M.a[3], x, fmaf(M.a[4], y, M.a[5]));
    const float r2 = fmaf(M.a[6], x, fmaf(M.a[7], y, M.a[8]));
    const float q0 = fmaf(g, r0, M.t[0]), q1 = fmaf(g, r1, M.t[1]), z = fmaf(g, r2, M.t[2]);
    const float zq = z + kEps;
    const bool persp = fabsf(z) > kEps;
    const float u = rintf(persp ? q0 / zq : q0), v = rintf(persp ? q1 / zq : q1);          // half to even
    if (!(u >= 0.0f && u < (float)Ws && v >= 0.0f && v < (float)Hs)) return false;         // (NaN fails)
    const int ix = (int)u, iy = (int)v;
    if (ix >= Ws || iy >= Hs) return false;            // ((float)Ws may have rounded up)
    S = M.src[(size_t)iy * Ws + ix];
    if (!(valid_depth(S, Q.min_depth, Q.max_depth) && zq > 0.0f && zq < Q.occlusion * S)) return false;
    a2 = fma((double)M.a[6], (double)x, fma((double)M.a[7], (double)y, (double)M.a[8]));
    zp = fma(G.E[j], a2, (double)M.t[2]) + (double)kEps;
    return fabs(zp) < (double)INFINITY && zp > 0.0;
}

// rows [blockIdx.x][K][2]: the workgroup's sum and count per source.  RES: residual [B,K,H,W] is written too.
template <bool RES>
__global__ __launch_bounds__(kThreads) void mv_fwd_kernel(int K, int H, int W, int Hs, int Ws, int S_pool, int chunks,
                                                          const float* __restrict__ depth, const float* __restrict__ gt,
                                                          const float* __restrict__ alpha, const float* __restrict__ src_depth,
                                                          const int* __restrict__ src_index, const float* __restrict__ pairs,
                                                          Params Q, double* __restrict__ rows, float* __restrict__ residual)
{
    __shared__ double s_sum[kWaves][kMaxK];
    __shared__ int s_cnt[kWaves][kMaxK];
    const int t = threadIdx.x;
    const long long b = blockIdx.x / chunks;
    const int chunk = (int)(blockIdx.x - b * chunks);
    const long long P = (long long)H * W, Ps = (long long)Hs * Ws;
    const size_t base = (size_t)b * (size_t)P;
    const Group G = load_group(((long long)chunk * kThreads + t) * kVec, P, W, depth + base, gt + base, alpha ? alpha + base : nullptr, Q);
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        const Pair M = pair_of(b, k, K, Ps, S_pool, src_depth, src_index, pairs);
        double sum = 0.0;
        int cnt = 0;
        Px4 res;
#pragma unroll
        for (int j = 0; j < kVec; ++j) res.v[j] = __builtin_nanf("");
        if (M.src) {
#pragma unroll
            for (int j = 0; j < kVec; ++j) {
                float S;
                double a2, zp;
                if (select(M, G, j, Hs, Ws, Q, S, a2, zp)) {
                    // the residual is rounded once, to the fp32 the map holds, and the sum adds that value: the sum IS the fp64
                    // sum of the residual map, whether the map is written or not
                    res.v[j] = (float)log_of(zp / (double)S);
                    sum += fabs((double)res.v[j]);
                    ++cnt;
                }
            }
        }
        if (RES) {
            float* out = residual + ((size_t)b * K + k) * (size_t)P;
            store4(out, G.p0, P, aligned16(out), res);
        }
        sum = wave_sum(sum);
        cnt = wave_sum(cnt);
        if ((t & (kWave - 1)) == 0) {
            s_sum[t / kWave][k] = sum;
            s_cnt[t / kWave][k] = cnt;
        }
    }
    __syncthreads();
    if (t < K) {
        double* row = rows + ((size_t)blockIdx.x * K + t) * 2;
        row[0] = waves_total(&s_sum[0][t], kMaxK);
        row[1] = (double)waves_total(&s_cnt[0][t], kMaxK);
    }
    static_assert(kMaxK <= kThreads, "the last step takes one thread per source");
}

// g_E = sum over the sources that select the pixel of g_sum[b,k] sgn(r) a[2] / z_p', then the chain through alpha
__global__ __launch_bounds__(kThreads) void mv_bwd_kernel(int K, int H, int W, int Hs, int Ws, int S_pool, int chunks,
                                                          const float* __restrict__ depth, const float* __restrict__ gt,
                                                          const float* __restrict__ alpha, const float* __restrict__ src_depth,
                                                          const int* __restrict__ src_index, const float* __restrict__ pairs,
                                                          Params Q, const float* __restrict__ g_sum, float* __restrict__ g_depth,
                                                          float* __restrict__ g_alpha)
{
    const long long b = blockIdx.x / chunks;
    const int chunk = (int)(blockIdx.x - b * chunks);
    const long long P = (long long)H * W, Ps = (long long)Hs * Ws;
    const size_t base = (size_t)b * (size_t)P;
    const Group G = load_group(((long long)chunk * kThreads + threadIdx.x) * kVec, P, W, depth + base, gt + base,
                               alpha ? alpha + base : nullptr, Q);
    if (G.p0 >= P) return;
    double gE[kVec];
    bool any[kVec];
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
        gE[j] = 0.0;
        any[j] = false;
    }
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        const Pair M = pair_of(b, k, K, Ps, S_pool, src_depth, src_index, pairs);
        if (!M.src) continue;
        const double gs = (double)g_sum[b * K + k];
#pragma unroll
        for (int j = 0; j < kVec; ++j) {
            float S;
            double a2, zp;
            if (select(M, G, j, Hs, Ws, Q, S, a2, zp)) {
                const double sgn = zp > (double)S ? 1.0 : (zp < (double)S ? -1.0 : 0.0);
                gE[j] = fma(gs * sgn, a2 / zp, gE[j]);
                any[j] = true;
            }
        }
    }
    Px4 gd, ga;
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
        gd.v[j] = 0.0f;
        ga.v[j] = 0.0f;
        if (any[j]) {                                  // (a pixel no source selects receives exactly 0, whatever its E)
            const double d = gE[j] / (double)G.m[j];
            gd.v[j] = (float)d;
            if (alpha && G.al[j] > Q.alpha_floor) ga.v[j] = (float)(-(d * G.E[j]));        // max(alpha, floor) = alpha here
        }
    }
    store4(g_depth + base, G.p0, P, aligned16(g_depth + base), gd);
    if (alpha) store4(g_alpha + base, G.p0, P, aligned16(g_alpha + base), ga);
}

// rows [blockIdx.x][3]: the workgroup's sums of d and d^2 and its count
__global__ __launch_bounds__(kThreads) void si_fwd_kernel(int H, int W, int chunks, const float* __restrict__ depth,
                                                          const float* __restrict__ gt, const float* __restrict__ alpha, Params Q,
                                                          double* __restrict__ rows)
{
    __shared__ double s_sum[kWaves][2];
    __shared__ int s_cnt[kWaves];
    const int t = threadIdx.x;
    const long long b = blockIdx.x / chunks;
    const int chunk = (int)(blockIdx.x - b * chunks);
    const long long P = (long long)H * W;
    const size_t base = (size_t)b * (size_t)P;
    const Group G = load_group(((long long)chunk * kThreads + t) * kVec, P, W, depth + base, gt + base, alpha ? alpha + base : nullptr, Q);
    double s1 = 0.0, s2 = 0.0;
    int n = 0;
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
        if (G.v0[j] && fabs(G.E[j]) < (double)INFINITY && G.E[j] > 0.0) {
            const double d = log_of((double)G.g[j] / G.E[j]);
            s1 += d;
            s2 = fma(d, d, s2);
            ++n;
        }
    }
    n = wave_sum(n);
    if ((t & (kWave - 1)) == 0) s_cnt[t / kWave] = n;
    double s[2] = {s1, s2};
    block_sum_waves<2>(s, &s_sum[0][0]);                   // (its barrier publishes s_cnt too)
    if (t == 0) {
        double* row = rows + (size_t)blockIdx.x * 3;
        row[0] = s[0];
        row[1] = s[1];
        row[2] = (double)waves_total(s_cnt, 1);
    }
}

// g_E = -(g_s1 + 2 d g_s2) / E on P, then the chain through alpha
__global__ __launch_bounds__(kThreads) void si_bwd_kernel(int H, int W, int chunks, const float* __restrict__ depth,
                                                          const float* __restrict__ gt, const float* __restrict__ alpha, Params Q,
                                                          const float* __restrict__ g_s1, const float* __restrict__ g_s2,
                                                          float* __restrict__ g_depth, float* __restrict__ g_alpha)
{
    const long long b = blockIdx.x / chunks;
    const int chunk = (int)(blockIdx.x - b * chunks);
    const long long P = (long long)H * W;
    const size_t base = (size_t)b * (size_t)P;
    const Group G = load_group(((long long)chunk * kThreads + threadIdx.x) * kVec, P, W, depth + base, gt + base,
                               alpha ? alpha + base : nullptr, Q);
    if (G.p0 >= P) return;
    const double c1 = (double)g_s1[b], c2 = (double)g_s2[b];
    Px4 gd, ga;
#pragma unroll
    for (int j = 0; j < kVec; ++j) {
        gd.v[j] = 0.0f;
        ga.v[j] = 0.0f;
        if (G.v0[j] && fabs(G.E[j]) < (double)INFINITY && G.E[j] > 0.0) {
            const double d = log_of((double)G.g[j] / G.E[j]);
            const double gE = -fma(2.0 * d, c2, c1) / G.E[j];
            const double gdd = gE / (double)G.m[j];
            gd.v[j] = (float)gdd;
            if (alpha && G.al[j] > Q.alpha_floor) ga.v[j] = (float)(-(gdd * G.E[j]));
        }
    }
    store4(g_depth + base, G.p0, P, aligned16(g_depth + base), gd);
    if (alpha) store4(g_alpha + base, G.p0, P, aligned16(g_alpha + base), ga);
}

struct Grid {
    int chunks;
    unsigned blocks;
};

// FS_OK, or why the sizes cannot run
int make_grid(int32_t B, int32_t H, int32_t W, Grid& g)
{
    if (B <= 0 || H <= 0 || W <= 0) return FS_ERR_INVALID_ARG;
    const long long P = (long long)H * W;
    if (P > 0x7fffffffLL) return FS_ERR_UNSUPPORTED;
    g.chunks = (int)((P + kChunk - 1) / kChunk);
    const long long blocks = (long long)B * g.chunks;
    if (blocks > 0x7fffffffLL) return FS_ERR_UNSUPPORTED;
    g.blocks = (unsigned)blocks;
    return FS_OK;
}

bool make_params(float occlusion, float min_depth, float max_depth, float alpha_floor, Params& Q)
{
    if (occlusion != occlusion || min_depth != min_depth || max_depth != max_depth) return false;
    if (!(alpha_floor > 0.0f && alpha_floor < INFINITY)) return false;
    Q = Params{occlusion, min_depth, max_depth, alpha_floor};
    return true;
}

// the checks the two multi-view entry points share
int check_mv(int32_t B, int32_t K, int32_t H, int32_t W, int32_t Hs, int32_t Ws, int32_t S_pool, const float* depth, const float* gt,
             const float* src_depth, const int32_t* src_index, const float* pairs, Grid& g)
{
    if (K <= 0 || Hs <= 0 || Ws <= 0 || (src_index && S_pool <= 0) || !depth || !gt || !src_depth || !pairs)
        return FS_ERR_INVALID_ARG;
    if (const int st = make_grid(B, H, W, g)) return st;
    if (K > kMaxK || (long long)Hs * Ws > 0x7fffffffLL || (long long)B * K > 0x7fffffffLL) return FS_ERR_UNSUPPORTED;
    return FS_OK;
}

}  // namespace

}  // namespace fs

using namespace fs;

FS_API int fs_mvdepth_api_version(void) { return FS_MVDEPTH_API_VERSION; }

FS_API size_t fs_mvdepth_scratch_bytes(int32_t B, int32_t K, int32_t H, int32_t W)
{
    Grid g;
    if (K < 0 || K > kMaxK || make_grid(B, H, W, g) != FS_OK) return 0;
    const size_t doubles = K * 2 > 3 ? (size_t)K * 2 : 3;                 // per workgroup: K (sum, cnt) rows, or (s1, s2, n)
    return align_up((size_t)g.blocks * doubles * sizeof(double), 256);
}

FS_API int fs_mv_depth_forward(int32_t B, int32_t K, int32_t H, int32_t W, int32_t Hs, int32_t Ws, int32_t S_pool, const float* depth,
                               const float* gt, const float* alpha, const float* src_depth, const int32_t* src_index,
                               const float* pairs, float occlusion, float min_depth, float max_depth, float alpha_floor, double* sum,
                               double* cnt, float* residual, void* scratch, void* stream_)
{
    Grid g;
    Params Q;
    if (!make_params(occlusion, min_depth, max_depth, alpha_floor, Q) || !sum || !cnt || !scratch) return FS_ERR_INVALID_ARG;
    if (const int st = check_mv(B, K, H, W, Hs, Ws, S_pool, depth, gt, src_depth, src_index, pairs, g)) return st;
    hipStream_t st = (hipStream_t)stream_;
    double* rows = static_cast<double*>(scratch);
    if (residual)
        hipLaunchKernelGGL((mv_fwd_kernel<true>), dim3(g.blocks), dim3(kThreads), 0, st, K, H, W, Hs, Ws, S_pool, g.chunks, depth, gt,
                           alpha, src_depth, (const int*)src_index, pairs, Q, rows, residual);
    else
        hipLaunchKernelGGL((mv_fwd_kernel<false>), dim3(g.blocks), dim3(kThreads), 0, st, K, H, W, Hs, Ws, S_pool, g.chunks, depth, gt,
                           alpha, src_depth, (const int*)src_index, pairs, Q, rows, residual);
    hipLaunchKernelGGL((finalize_rows_kernel<2, BlockSum::kWaves, false>), dim3((unsigned)(B * K)), dim3(kThreads), 0, st, g.chunks, K,
                       (const double*)rows, RowOuts<2>{{sum, cnt}, {}, 1});
    FS_CHECK_LAUNCH("mv_depth_forward");
    return FS_OK;
}

FS_API int fs_mv_depth_backward(int32_t B, int32_t K, int32_t H, int32_t W, int32_t Hs, int32_t Ws, int32_t S_pool, const float* depth,
                                const float* gt, const float* alpha, const float* src_depth, const int32_t* src_index,
                                const float* pairs, float occlusion, float min_depth, float max_depth, float alpha_floor,
                                const float* g_sum, float* g_depth, float* g_alpha, void* stream_)
{
    Grid g;
    Params Q;
    if (!make_params(occlusion, min_depth, max_depth, alpha_floor, Q) || !g_sum || !g_depth || (alpha != nullptr) != (g_alpha != nullptr))
        return FS_ERR_INVALID_ARG;
    if (const int st = check_mv(B, K, H, W, Hs, Ws, S_pool, depth, gt, src_depth, src_index, pairs, g)) return st;
    hipLaunchKernelGGL(mv_bwd_kernel, dim3(g.blocks), dim3(kThreads), 0, (hipStream_t)stream_, K, H, W, Hs, Ws, S_pool, g.chunks, depth,
                       gt, alpha, src_depth, (const int*)src_index, pairs, Q, g_sum, g_depth, g_alpha);
    FS_CHECK_LAUNCH("mv_depth_backward");
    return FS_OK;
}

FS_API int fs_si_depth_forward(int32_t B, int32_t H, int32_t W, const float* depth, const float* gt, const float* alpha,
                               float min_depth, float max_depth, float alpha_floor, double* s1, double* s2, double* n, void* scratch,
                               void* stream_)
{
    Grid g;
    Params Q;
    if (!make_params(1.0f, min_depth, max_depth, alpha_floor, Q) || !depth || !gt || !s1 || !s2 || !n || !scratch)
        return FS_ERR_INVALID_ARG;
    if (const int st = make_grid(B, H, W, g)) return st;
    hipStream_t st = (hipStream_t)stream_;
    double* rows = static_cast<double*>(scratch);
    hipLaunchKernelGGL(si_fwd_kernel, dim3(g.blocks), dim3(kThreads), 0, st, H, W, g.chunks, depth, gt, alpha, Q, rows);
    hipLaunchKernelGGL((finalize_rows_kernel<3, BlockSum::kWaves, false>), dim3((unsigned)B), dim3(kThreads), 0, st, g.chunks, 1,
                       (const double*)rows, RowOuts<3>{{s1, s2, n}, {}, 1});
    FS_CHECK_LAUNCH("si_depth_forward");
    return FS_OK;
}

FS_API int fs_si_depth_backward(int32_t B, int32_t H, int32_t W, const float* depth, const float* gt, const float* alpha,
                                float min_depth, float max_depth, float alpha_floor, const float* g_s1, const float* g_s2,
                                float* g_depth, float* g_alpha, void* stream_)
{
    Grid g;
    Params Q;
    if (!make_params(1.0f, min_depth, max_depth, alpha_floor, Q) || !depth || !gt || !g_s1 || !g_s2 || !g_depth ||
        (alpha != nullptr) != (g_alpha != nullptr))
        return FS_ERR_INVALID_ARG;
    if (const int st = make_grid(B, H, W, g)) return st;
    hipLaunchKernelGGL(si_bwd_kernel, dim3(g.blocks), dim3(kThreads), 0, (hipStream_t)stream_, H, W, g.chunks, depth, gt, alpha, Q, g_s1,
                       g_s2, g_depth, g_alpha);
    FS_CHECK_LAUNCH("si_depth_backward");
    return FS_OK;
}
