// gaussian_pose.hip -- gradients with respect to a similarity or a camera pose (include/freesplat_amd_pose.h): the contraction of
// per-Gaussian values and gradients with the generators of Sim(3), fs_sim3_tangent.
//
// The call moves bytes: at degree 3 a Gaussian is 2 x 58 floats in against about 300 fp64 multiply-adds.  As in
// gaussian_transform.hip a thread owns four consecutive Gaussians, whose floats are a multiple of four in every array, so a run
// starts at a multiple of 16 bytes from its array's base: an array whose base is 16-byte aligned goes through float4 loads, any
// other array and the last, partial run through dword loads with a bound check.  The harmonics are taken one Gaussian at a time
// (12, 27 or 48 floats of values and as many of gradients; at M = 9 through the 16-byte words that cover the 27), so that no
// more than one Gaussian's coefficients are live.  Which path loaded a value changes nothing about the arithmetic.
//
// Sums: products of fp32 values formed in fp64 (exact), each thread's seven fp64 sums in a fixed order, block_sum_waves
// (fs_reduce.h) per workgroup, one row of partials per (id, workgroup) in the caller's scratch, and finalize_rows_kernel per
// id.  The grid's second dimension runs over the ids: workgroup (b, v) takes the
// Gaussians of chunk b whose id is v.  Ids come in long runs (one view after another), so all but one or two of a chunk's V
// workgroups find no Gaussian of theirs, write a row of zeros after reading 8 KB of ids and leave; a thread none of whose
// four Gaussians match loads nothing.  What workgroup (b, v) adds up depends on nothing but the positions and values of the
// Gaussians with id v in chunk b, so any id pattern gives the same bits as those Gaussians alone.  No float atomics, no
// workgroup waits on another.
//
// The SH generators G_{l,k} = d D_l(exp(theta [e_k]x)) / d theta at 0 of the rasterizer's basis are antisymmetric and sparse:
// 24 entries above the diagonals of the nine matrices, with the closed forms 1, 2, 3, sqrt(3), sqrt(3/2), sqrt(5/2), sqrt(6).
// They are compile-time constants here (kGen); the contraction g^T G c runs over those entries only, as
// G[i][j] (g_i c_j - g_j c_i) summed over the three colour channels first.
#include "fs_reduce.h"

#include <utility>

#include "../../include/freesplat_amd_pose.h"

namespace fs {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kSumWaves;
constexpr int kGroup = 4;                            // Gaussians of a thread
constexpr int kChunk = kThreads * kGroup;            // Gaussians of a workgroup
constexpr int kSums = FS_SIM3_TANGENT_DIM;           // (u, omega, sigma)
constexpr int kFlagMask = FS_TRANSFORM_SH_CHANNEL_MAJOR | FS_TRANSFORM_QUAT_XYZW | FS_TRANSFORM_COV_FULL;

// G_{l,k}[i][j] = g = -G_{l,k}[j][i] with i < j; every other entry is 0
struct Gen {
    int k, l, i, j;
    double g;
};
constexpr double kS3 = 1.7320508075688772, kS32 = 1.2247448713915890, kS52 = 1.5811388300841898, kS6 = 2.4494897427831779;
constexpr int kGens = 24;
constexpr Gen kGen[kGens] = {
    {0, 1, 0, 1, 1.0},  {0, 2, 0, 3, 1.0},   {0, 2, 1, 2, kS3},   {0, 2, 1, 4, 1.0}, {0, 3, 0, 5, kS32}, {0, 3, 1, 4, kS52},
    {0, 3, 1, 6, kS32}, {0, 3, 2, 3, kS6},   {0, 3, 2, 5, kS52},
    {1, 1, 1, 2, 1.0},  {1, 2, 0, 1, -1.0},  {1, 2, 2, 3, kS3},   {1, 2, 3, 4, 1.0}, {1, 3, 0, 1, -kS32}, {1, 3, 1, 2, -kS52},
    {1, 3, 3, 4, kS6},  {1, 3, 4, 5, kS52},  {1, 3, 5, 6, kS32},
    {2, 1, 0, 2, 1.0},  {2, 2, 0, 4, 2.0},   {2, 2, 1, 3, 1.0},   {2, 3, 0, 6, 3.0}, {2, 3, 1, 5, 2.0},  {2, 3, 2, 4, 1.0}};

template <int... Is, class F>
__device__ __forceinline__ void static_for(std::integer_sequence<int, Is...>, F&& f)
{
    (f(std::integral_constant<int, Is>{}), ...);
}

// the W floats of Gaussian J of the run that starts at float offset `off` (a multiple of four): floats [J W, J W + W) of the
// run, through the 16-byte words that cover them when the array is aligned and those words lie inside it, else one by one.
// The Gaussian exists (the caller checked), so its own floats are inside the array on either path.
template <int W, int J>
__device__ __forceinline__ void load_gaussian(const float* __restrict__ base, size_t off, size_t total, bool aligned, float (&r)[W])
{
    constexpr int first = J * W, a0 = first & ~3, a1 = (first + W + 3) & ~3, K = (a1 - a0) / 4;
    if (aligned && off + a1 <= total) {
        float w[K * 4];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float4 q = *reinterpret_cast<const float4*>(base + off + a0 + 4 * k);
            w[4 * k] = q.x; w[4 * k + 1] = q.y; w[4 * k + 2] = q.z; w[4 * k + 3] = q.w;
        }
#pragma unroll
        for (int e = 0; e < W; ++e) r[e] = w[first - a0 + e];
    } else {
#pragma unroll
        for (int e = 0; e < W; ++e) r[e] = base[off + first + e];
    }
}

// ---- the terms of one Gaussian; s = (u, omega, sigma) -------------------------------------------------------------------------

// tau_u += g; with the mean: tau_omega += mu x g, tau_sigma += mu . g
__device__ __forceinline__ void mean_term(const float* m, const float* g_, bool with_mean, double (&s)[kSums])
{
    const double gx = g_[0], gy = g_[1], gz = g_[2];
    s[0] += gx;
    s[1] += gy;
    s[2] += gz;
    if (with_mean) {
        const double x = m[0], y = m[1], z = m[2];
        s[3] = fma(-z, gy, fma(y, gz, s[3]));
        s[4] = fma(-x, gz, fma(z, gx, s[4]));
        s[5] = fma(-y, gx, fma(x, gy, s[5]));
        s[6] = fma(z, gz, fma(y, gy, fma(x, gx, s[6])));
    }
}

__device__ __forceinline__ void scale_term(const float* a, const float* g_, double (&s)[kSums])
{
    s[6] = fma((double)a[2], (double)g_[2], fma((double)a[1], (double)g_[1], fma((double)a[0], (double)g_[0], s[6])));
}

// tau_omega += 1/2 (w g_v - g_w v + v x g_v) for q = (w, v), g = (g_w, g_v): g . (1/2 (0, e_k) (x) q) written out
__device__ __forceinline__ void quat_term(const float* q, const float* g_, bool xyzw, double (&s)[kSums])
{
    const double w = xyzw ? q[3] : q[0], x = xyzw ? q[0] : q[1], y = xyzw ? q[1] : q[2], z = xyzw ? q[2] : q[3];
    const double gw = xyzw ? g_[3] : g_[0], gx = xyzw ? g_[0] : g_[1], gy = xyzw ? g_[1] : g_[2], gz = xyzw ? g_[2] : g_[3];
    const double tx = fma(-z, gy, fma(y, gz, fma(-gw, x, w * gx)));
    const double ty = fma(-x, gz, fma(z, gx, fma(-gw, y, w * gy)));
    const double tz = fma(-y, gx, fma(x, gy, fma(-gw, z, w * gz)));
    s[3] = fma(0.5, tx, s[3]);
    s[4] = fma(0.5, ty, s[4]);
    s[5] = fma(0.5, tz, s[5]);
}

// tau_omega,k += <G, [e_k]x S - S [e_k]x> = a_k(S G^T - G^T S), a(A) = (A_12 - A_21, A_20 - A_02, A_01 - A_10);
// tau_sigma += 2 <G, S>.  Six entries: S symmetric, G the symmetric matrix with the off-diagonal gradients halved (exact), whose
// inner product with a symmetric matrix is the contraction over the six stored entries.
template <bool FULL>
__device__ __forceinline__ void cov_term(const float* c, const float* g_, double (&s)[kSums])
{
    double S[9], G[9];
    if constexpr (FULL) {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            S[k] = c[k];
            G[k] = g_[k];
        }
    } else {
        S[0] = c[0]; S[1] = S[3] = c[1]; S[2] = S[6] = c[2]; S[4] = c[3]; S[5] = S[7] = c[4]; S[8] = c[5];
        G[0] = g_[0]; G[1] = G[3] = 0.5 * (double)g_[1]; G[2] = G[6] = 0.5 * (double)g_[2]; G[4] = g_[3];
        G[5] = G[7] = 0.5 * (double)g_[4]; G[8] = g_[5];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = (k + 1) % 3, j = (k + 2) % 3;
        double a = s[3 + k];
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            a = fma(S[i * 3 + m], G[j * 3 + m], a);         //  (S G^T)_ij
            a = fma(-G[m * 3 + i], S[m * 3 + j], a);        // -(G^T S)_ij
            a = fma(-S[j * 3 + m], G[i * 3 + m], a);        // -(S G^T)_ji
            a = fma(G[m * 3 + j], S[m * 3 + i], a);         //  (G^T S)_ji
        }
        s[3 + k] = a;
    }
    double d = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) d = fma(G[k], S[k], d);
    s[6] = fma(2.0, d, s[6]);
}

// tau_omega,k += sum over bands and channels of g_l^T G_{l,k} c_l.  c, g: the 3 M coefficients of one Gaussian, [M][3] or (CM) [3][M]
template <int M, bool CM>
__device__ __forceinline__ void sh_term(const float (&c)[3 * M], const float (&g_)[3 * M], double (&s)[kSums])
{
    constexpr int DEG = M == 16 ? 3 : M == 9 ? 2 : M == 4 ? 1 : 0;
    static_for(std::make_integer_sequence<int, kGens>{}, [&](auto p) {
        constexpr Gen e = kGen[decltype(p)::value];
        if constexpr (e.l <= DEG) {
            constexpr int a = e.l * e.l + e.i, b = e.l * e.l + e.j;
            double w = 0.0;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int ia = CM ? ch * M + a : a * 3 + ch, ib = CM ? ch * M + b : b * 3 + ch;
                w = fma(-(double)g_[ib], (double)c[ia], fma((double)g_[ia], (double)c[ib], w));
            }
            s[3 + e.k] = fma(e.g, w, s[3 + e.k]);
        }
    });
}

// one array of W floats per Gaussian: the thread's run of four through f(values, gradients) for the Gaussians that are on
template <int W, class F>
__device__ __forceinline__ void geom_array(const float* __restrict__ vals, const float* __restrict__ grads, long long n0, int N,
                                           const bool (&on)[kGroup], F&& f)
{
    constexpr int S = kGroup * W;
    const size_t total = (size_t)N * W, off = (size_t)n0 * W;
    float a[S], g_[S];
    load_run<S>(grads, off, total, aligned16(grads), g_);
    if (vals) {
        load_run<S>(vals, off, total, aligned16(vals), a);
    } else {
#pragma unroll
        for (int k = 0; k < S; ++k) a[k] = 0.0f;
    }
#pragma unroll
    for (int j = 0; j < kGroup; ++j)
        if (on[j]) f(a + j * W, g_ + j * W);
}

// workgroup (b, v): row v * gridDim.x + b of `rows`, the seven sums over the Gaussians of chunk b whose id is v
template <int M, bool CM, bool COV_FULL>
__global__ __launch_bounds__(kThreads) void tangent_kernel(int N, int xyzw_, const long long* __restrict__ ids,
                                                           const float* __restrict__ means, const float* __restrict__ scales,
                                                           const float* __restrict__ rot, const float* __restrict__ cov,
                                                           const float* __restrict__ shs, const float* __restrict__ g_means,
                                                           const float* __restrict__ g_scales, const float* __restrict__ g_rot,
                                                           const float* __restrict__ g_cov, const float* __restrict__ g_shs,
                                                           double* __restrict__ rows)
{
    __shared__ double s_red[kWaves * kSums];
    const long long v = blockIdx.y;
    const long long n0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * kGroup;
    double* __restrict__ row = rows + ((size_t)v * gridDim.x + blockIdx.x) * kSums;
    bool on[kGroup], any = false;
#pragma unroll
    for (int j = 0; j < kGroup; ++j) {
        const long long n = n0 + j;
        on[j] = n < N && (!ids || ids[n] == v);
        any |= on[j];
    }
    if (!__syncthreads_or(any ? 1 : 0)) {                                   // (the same for the whole workgroup)
        if (threadIdx.x < kSums) row[threadIdx.x] = 0.0;
        return;
    }
    double s[kSums];
#pragma unroll
    for (int f = 0; f < kSums; ++f) s[f] = 0.0;
    if (any) {
        const bool xyzw = xyzw_ != 0, with_mean = means != nullptr;
        if (g_means) geom_array<3>(means, g_means, n0, N, on, [&](const float* a, const float* g_) { mean_term(a, g_, with_mean, s); });
        if (g_scales) geom_array<3>(scales, g_scales, n0, N, on, [&](const float* a, const float* g_) { scale_term(a, g_, s); });
        if (g_rot) geom_array<4>(rot, g_rot, n0, N, on, [&](const float* a, const float* g_) { quat_term(a, g_, xyzw, s); });
        if (g_cov)
            geom_array<COV_FULL ? 9 : 6>(cov, g_cov, n0, N, on, [&](const float* a, const float* g_) { cov_term<COV_FULL>(a, g_, s); });
        if constexpr (M > 1) {
            if (g_shs) {
                constexpr int W = 3 * M;
                const size_t total = (size_t)N * W, off = (size_t)n0 * W;
                const bool ca = aligned16(shs), ga = aligned16(g_shs);
                static_for(std::make_integer_sequence<int, kGroup>{}, [&](auto jj) {
                    constexpr int J = decltype(jj)::value;
                    if (on[J]) {
                        float c[W], g_[W];
                        load_gaussian<W, J>(shs, off, total, ca, c);
                        load_gaussian<W, J>(g_shs, off, total, ga, g_);
                        sh_term<M, CM>(c, g_, s);
                    }
                });
            }
        }
    }
    block_sum_waves<kSums>(s, s_red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int f = 0; f < kSums; ++f) row[f] = s[f];
}

bool valid_m(int32_t M) { return M == 1 || M == 4 || M == 9 || M == 16; }

int chunks_of(int32_t N) { return (int)(((long long)N + kChunk - 1) / kChunk); }

struct Args {
    int N, xyzw;
    const long long* ids;
    const float *means, *scales, *rot, *cov, *shs, *g_means, *g_scales, *g_rot, *g_cov, *g_shs;
    double* rows;
};

template <int M, bool CM>
void launch(bool cov_full, dim3 grid, hipStream_t st, const Args& a)
{
    if (cov_full)
        hipLaunchKernelGGL((tangent_kernel<M, CM, true>), grid, dim3(kThreads), 0, st, a.N, a.xyzw, a.ids, a.means, a.scales, a.rot, a.cov,
                           a.shs, a.g_means, a.g_scales, a.g_rot, a.g_cov, a.g_shs, a.rows);
    else
        hipLaunchKernelGGL((tangent_kernel<M, CM, false>), grid, dim3(kThreads), 0, st, a.N, a.xyzw, a.ids, a.means, a.scales, a.rot, a.cov,
                           a.shs, a.g_means, a.g_scales, a.g_rot, a.g_cov, a.g_shs, a.rows);
}

template <int M>
void launch_m(bool cm, bool cov_full, dim3 grid, hipStream_t st, const Args& a)
{
    if (cm)
        launch<M, true>(cov_full, grid, st, a);
    else
        launch<M, false>(cov_full, grid, st, a);
}

}  // namespace

}  // namespace fs

using namespace fs;

FS_API int fs_pose_api_version(void) { return FS_POSE_API_VERSION; }

FS_API size_t fs_sim3_tangent_scratch_bytes(int32_t N, int32_t V)
{
    if (N <= 0 || V < 1 || V > FS_SIM3_MAX_ROWS) return 0;
    return (size_t)V * chunks_of(N) * kSums * sizeof(double);
}

FS_API int fs_sim3_sh_generators(double* out)
{
    if (!out) return FS_ERR_INVALID_ARG;
    constexpr int kOff[3] = {0, 9, 34};
    for (int k = 0; k < 3 * FS_SIM3_SH_GENERATOR_DOUBLES; ++k) out[k] = 0.0;
    for (const Gen& e : kGen) {
        const int n = 2 * e.l + 1;
        double* G = out + e.k * FS_SIM3_SH_GENERATOR_DOUBLES + kOff[e.l - 1];
        G[e.i * n + e.j] = e.g;
        G[e.j * n + e.i] = -e.g;
    }
    return FS_OK;
}

FS_API int fs_sim3_tangent(int32_t N, int32_t M, int32_t V, int32_t flags, const int64_t* ids, const float* means, const float* scales,
                           const float* rotations, const float* cov, const float* shs, const float* g_means, const float* g_scales,
                           const float* g_rotations, const float* g_cov, const float* g_shs, double* out, void* scratch,
                           size_t scratch_bytes, void* stream_)
{
    if (N <= 0 || !valid_m(M) || V < 1 || V > FS_SIM3_MAX_ROWS || (flags & ~kFlagMask) || (!ids && V != 1)) return FS_ERR_INVALID_ARG;
    if ((means && !g_means) || (!scales != !g_scales) || (!rotations != !g_rotations) || (!cov != !g_cov) || (!shs != !g_shs))
        return FS_ERR_INVALID_ARG;
    if (!g_means && !g_scales && !g_rotations && !g_cov && !g_shs) return FS_ERR_INVALID_ARG;
    if (!out || !scratch || scratch_bytes < fs_sim3_tangent_scratch_bytes(N, V)) return FS_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream_;
    const int blocks = chunks_of(N);
    const dim3 grid((unsigned)blocks, (unsigned)V);
    const Args a = {N, (flags & FS_TRANSFORM_QUAT_XYZW) ? 1 : 0, (const long long*)ids, means, scales, rotations, cov, shs,
                    g_means, g_scales, g_rotations, g_cov, g_shs, (double*)scratch};
    const bool cm = (flags & FS_TRANSFORM_SH_CHANNEL_MAJOR) != 0, cov_full = (flags & FS_TRANSFORM_COV_FULL) != 0;
    switch (M) {
        case 1: launch_m<1>(false, cov_full, grid, st, a); break;          // band 0 does not turn: the harmonics are not read
        case 4: launch_m<4>(cm, cov_full, grid, st, a); break;
        case 9: launch_m<9>(cm, cov_full, grid, st, a); break;
        default: launch_m<16>(cm, cov_full, grid, st, a); break;
    }
    RowOuts<kSums> outs = {};                               // out [V][kSums]
    for (int f = 0; f < kSums; ++f) outs.out[f] = out + f;
    outs.stride = kSums;
    hipLaunchKernelGGL((finalize_rows_kernel<kSums, BlockSum::kWaves, false>), dim3((unsigned)V), dim3(kThreads), 0, st, blocks, 1,
                       (const double*)scratch, outs);
    FS_CHECK_LAUNCH("sim3_tangent");
    return FS_OK;
}
