// fs_reduce.h -- device helpers the loss / metric / transform kernels share: the two fixed-order block reductions, the
// finalize kernel that adds a view's partial rows, the 16-byte access helpers and the depth validity tests.  A new op starts
// from these (and ssim_pass.h), not from a copy of another op's helpers (DESIGN.md "Helper headers").
//
// Every reduction here is over a workgroup of kSumThreads = 256 threads = 4 wavefronts and adds doubles in ONE association
// order that depends on nothing but the thread index.  The tests' bit-level claims (a view's result is the same bits alone or
// inside a batch, on any stream, at any alignment) rest on these orders: changing either changes result bits.
//
//   block_sum_tree   LDS tree.  Thread t's value goes to slot t; for s = 128, 64, .. 1: slot t += slot t + s (t < s).  Every
//                    thread ends with the total.  Scratch [F][256] doubles.  Used by metrics.hip, ssim_loss.hip,
//                    depth_loss.hip, normals_loss.hip.
//   block_sum_waves  Inside each wavefront six __shfl_down steps (offsets 32, 16, .. 1: lane l += lane l + offset), then thread 0
//                    adds the four wavefronts' totals as ((w0 + w1) + w2) + w3.  Only thread 0 ends with the total.  Scratch
//                    [4][F] doubles.  Used by exposure.hip, mv_depth_loss.hip, gaussian_pose.hip.
#pragma once
#include "fs_common.h"

#include <math.h>

namespace fs {

constexpr int kSumThreads = 256;
constexpr int kSumWaves = kSumThreads / kWave;
static_assert(kSumWaves == 4, "block_sum_waves and waves_total add four wavefronts");

template <int F>
__device__ __forceinline__ void block_sum_tree(double (&v)[F], double* s_red /* [F][kSumThreads] */)
{
    const int t = threadIdx.x;
#pragma unroll
    for (int f = 0; f < F; ++f) s_red[f * kSumThreads + t] = v[f];
    __syncthreads();
    for (int s = kSumThreads / 2; s > 0; s >>= 1) {
        if (t < s)
#pragma unroll
            for (int f = 0; f < F; ++f) s_red[f * kSumThreads + t] += s_red[f * kSumThreads + t + s];
        __syncthreads();
    }
#pragma unroll
    for (int f = 0; f < F; ++f) v[f] = s_red[f * kSumThreads];
}

// fixed-order sum over the 64 lanes of a wavefront (double, or int for counts); the total is valid in lane 0
template <class T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;
}

// the four wavefronts' totals s[0], s[stride], s[2 stride], s[3 stride], in order
template <class T>
__device__ __forceinline__ T waves_total(const T* s, int stride)
{
    return ((s[0] + s[stride]) + s[2 * stride]) + s[3 * stride];
}

// One __syncthreads() lies between the wavefronts' stores and thread 0's reads: what a caller wrote to LDS before the call
// (an integer count per wavefront, say) is visible to thread 0 after it.  The two steps are wave_sum and waves_total written
// out: called through them, exposure.hip's fit finalizer compiles to 72 VGPRs instead of 64.
template <int F>
__device__ __forceinline__ void block_sum_waves(double (&v)[F], double* s_red /* [kSumWaves][F] */)
{
    const int t = threadIdx.x;
#pragma unroll
    for (int f = 0; f < F; ++f)
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) v[f] += __shfl_down(v[f], off, kWave);
    if ((t & (kWave - 1)) == 0)
#pragma unroll
        for (int f = 0; f < F; ++f) s_red[(t / kWave) * F + f] = v[f];
    __syncthreads();
    if (t == 0)
#pragma unroll
        for (int f = 0; f < F; ++f) v[f] = ((s_red[f] + s_red[F + f]) + s_red[2 * F + f]) + s_red[3 * F + f];
}

// ---- "one workgroup adds a view's partial rows" ---------------------------------------------------------------------------------

enum class BlockSum { kTree, kWaves };

// out[f][blockIdx.x * stride] receives field f, times scale[f] when the kernel is instantiated with SCALE
template <int F>
struct RowOuts {
    double* out[F];
    double scale[F];
    int stride;
};

namespace {

// One workgroup per (view, group g of G), blockIdx.x = view * G + g.  rows [view][K][G][F]: the workgroup's K rows are strided
// over the threads in index order (thread t adds rows t, t + 256, ..), then the block sum of FORM.
template <int F, BlockSum FORM, bool SCALE>
__global__ __launch_bounds__(kSumThreads) void finalize_rows_kernel(int K, int G, const double* __restrict__ rows, RowOuts<F> outs)
{
    __shared__ double s_red[FORM == BlockSum::kTree ? F * kSumThreads : kSumWaves * F];
    const long long view = blockIdx.x / G;
    const int g = (int)(blockIdx.x - view * G);
    const double* r = rows + ((size_t)view * K * G + g) * F;
    double v[F];
#pragma unroll
    for (int f = 0; f < F; ++f) v[f] = 0.0;
    for (int k = threadIdx.x; k < K; k += kSumThreads)
#pragma unroll
        for (int f = 0; f < F; ++f) v[f] += r[(size_t)k * G * F + f];
    if constexpr (FORM == BlockSum::kTree)
        block_sum_tree<F>(v, s_red);
    else
        block_sum_waves<F>(v, s_red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int f = 0; f < F; ++f) outs.out[f][(size_t)blockIdx.x * outs.stride] = SCALE ? v[f] * outs.scale[f] : v[f];
}

}  // namespace

// ---- 16-byte accesses -------------------------------------------------------------------------------------------------------------
// A thread owns four consecutive floats that start at a multiple of four from the array's base, so whether they can go through
// one 16-byte access depends on the base address alone.  Which path moved a value changes nothing about its arithmetic.

__host__ __device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct Px4 {
    float v[4];
};

// the four pixels p0 .. p0 + 3 of a plane; a pixel at or beyond P reads nothing and is 0
__device__ __forceinline__ Px4 load4(const float* __restrict__ plane, long long p0, long long P, bool aligned)
{
    Px4 r;
    if (aligned && p0 + 4 <= P) {
        const float4 q = *reinterpret_cast<const float4*>(plane + p0);
        r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) r.v[j] = p0 + j < P ? plane[p0 + j] : 0.0f;
    }
    return r;
}

__device__ __forceinline__ void store4(float* __restrict__ plane, long long p0, long long P, bool aligned, const Px4& r)
{
    if (aligned && p0 + 4 <= P) {
        *reinterpret_cast<float4*>(plane + p0) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + j < P) plane[p0 + j] = r.v[j];
    }
}

// the S floats (S a multiple of four) at float offset `off` of an array of `total` floats; a float at or beyond `total` reads
// nothing and is 0.  (No __restrict__: gaussian_transform.hip transforms arrays in place.)
template <int S>
__device__ __forceinline__ void load_run(const float* base, size_t off, size_t total, bool aligned, float (&r)[S])
{
    static_assert(S % 4 == 0, "a run is whole 16-byte words");
    if (aligned && off + S <= total) {
#pragma unroll
        for (int k = 0; k < S / 4; ++k) {
            const float4 q = *reinterpret_cast<const float4*>(base + off + 4 * k);
            r[4 * k] = q.x; r[4 * k + 1] = q.y; r[4 * k + 2] = q.z; r[4 * k + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < S; ++k) r[k] = off + k < total ? base[off + k] : 0.0f;
    }
}

// ---- depth maps -------------------------------------------------------------------------------------------------------------------

// a sensor depth counts: finite and inside (min_depth, max_depth).  Holes may be NaN, +-inf, 0 or negative.
__device__ __forceinline__ bool valid_depth(float g, float min_depth, float max_depth)
{
    return fabsf(g) < INFINITY && g > min_depth && g < max_depth;       // (NaN fails every comparison)
}

// expected depth of a pixel from the rasterizer's accumulated depth and alpha, in T = float or double
template <class T>
__device__ __forceinline__ T expected_depth(float d, float alpha, bool has_alpha, float alpha_floor)
{
    return has_alpha ? (T)d / (T)fmaxf(alpha, alpha_floor) : (T)d;
}

}  // namespace fs
