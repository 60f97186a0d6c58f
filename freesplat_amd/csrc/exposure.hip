// exposure.hip -- per-view exposure compensation (include/freesplat_amd_exposure.h): the affine colour op out = A x + b on
// [B,3,H,W] images with a [V,3,4] parameter array, its backward (g_image and g_params) and the least-squares affine colour fit.
//
// All three ops move bytes: 3 to 22 multiply-adds per pixel against 24 to 36 bytes.  One thread owns groups of four consecutive
// pixels; a group starts at a pixel index that is a multiple of four, so whether a plane can be accessed with 16-byte loads
// and stores depends on the plane's base address alone and is the same for the whole workgroup: a plane whose base is 16-byte
// aligned goes through float4, any other plane (an array 4 bytes off a boundary, a pixel count that is no multiple of four)
// and the last, partial group of every plane go through dword accesses with a bound check.  Which path loaded a pixel changes
// nothing about its arithmetic or about the thread that owns it: the per-pixel chain is the same explicit fmaf sequence and
// the per-thread sums run over the same pixels in the same order, so every output has the same bits at any alignment.
//
// A workgroup owns kChunk consecutive pixels of ONE batch entry (blockIdx.x = entry * chunks + chunk): the entry's view id and
// the 12 parameters of that view are wave-uniform and are read once per workgroup with scalar loads, not per pixel.  An id
// outside [0, V) turns the workgroup into a copy and keeps it away from the parameter array.
//
// Sums (g_params: 12, fit: 22): products of fp32 values formed in fp64 (exact), each thread's fp64 sums in a fixed order,
// block_sum_waves (fs_reduce.h) per workgroup, one row of partials per workgroup in the caller's scratch, and one finalize
// workgroup per VIEW that walks the entries in index order, takes those whose id equals its view and
// adds their rows in row order (in the fit, one thread of it then does the 4 x 4 Cholesky solve).  The partition depends on
// (H, W) only.  No float atomics, no workgroup waits on another.
#include "fs_reduce.h"

#include "../../include/freesplat_amd_exposure.h"

namespace fs {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kSumWaves;
constexpr int kVec = 4;                              // pixels of a group: one 16-byte access per plane
constexpr int kIters = 4;                            // groups per thread
constexpr int kGroups = kThreads * kIters;           // groups per workgroup
constexpr int kChunk = kGroups * kVec;               // pixels per workgroup (freesplat_amd/exposure.py CHUNK)
constexpr int kGradSums = 12, kFitSums = 22;         // doubles per partial row

// fit sums: M = sum X X^T as {x0x0, x0x1, x0x2, x0, x1x1, x1x2, x1, x2x2, x2, 1}, then R = sum X y^T as [k][c], k = 3 being y itself
constexpr int kCnt = 9, kR = 10;

// the mask bytes of the four pixels (nonzero = use); a pixel at or beyond P is 0
__device__ __forceinline__ uint32_t load_mask4(const uint8_t* __restrict__ m, long long p0, long long P, bool aligned)
{
    if (aligned && p0 + kVec <= P) return *reinterpret_cast<const uint32_t*>(m + p0);
    uint32_t r = 0;
#pragma unroll
    for (int j = 0; j < kVec; ++j)
        if (p0 + j < P) r |= (uint32_t)m[p0 + j] << (8 * j);
    return r;
}

// what a workgroup knows of its batch entry: all of it wave-uniform
struct Entry {
    long long b;          // batch entry
    int chunk;            // chunk of the entry's pixels
    bool on;              // the entry's id names a view; false: pass through
    float a[12];          // that view's [3][4] row-major (A | b); untouched when !on
};

__device__ __forceinline__ Entry entry_of_block(int V, int chunks, const float* __restrict__ params,
                                                const long long* __restrict__ view_ids)
{
    Entry e;
    e.b = blockIdx.x / chunks;
    e.chunk = (int)(blockIdx.x - e.b * chunks);
    const long long id = view_ids ? view_ids[e.b] : e.b;
    e.on = id >= 0 && id < (long long)V;
    const float* q = params + (e.on ? id : 0) * 12;                  // (an id out of range never forms an address)
#pragma unroll
    for (int k = 0; k < 12; ++k) e.a[k] = q[k];
    return e;
}

// out = A x + b.  All of a thread's groups are loaded before the first is used.
__global__ __launch_bounds__(kThreads) void exposure_fwd_kernel(int V, long long P, int chunks, const float* __restrict__ image,
                                                                const float* __restrict__ params,
                                                                const long long* __restrict__ view_ids, float* __restrict__ out)
{
    const Entry e = entry_of_block(V, chunks, params, view_ids);
    const float* x[3];
    float* o[3];
    bool xa[3], oa[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        x[c] = image + ((size_t)e.b * 3 + c) * (size_t)P;
        o[c] = out + ((size_t)e.b * 3 + c) * (size_t)P;
        xa[c] = aligned16(x[c]);
        oa[c] = aligned16(o[c]);
    }
    const long long g0 = (long long)e.chunk * kGroups + threadIdx.x;
    Px4 in[kIters][3];
#pragma unroll
    for (int k = 0; k < kIters; ++k)
#pragma unroll
        for (int c = 0; c < 3; ++c) in[k][c] = load4(x[c], (g0 + k * kThreads) * kVec, P, xa[c]);
#pragma unroll
    for (int k = 0; k < kIters; ++k) {
        const long long p0 = (g0 + k * kThreads) * kVec;
        if (p0 >= P) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Px4 r;
#pragma unroll
            for (int j = 0; j < kVec; ++j) {
                const float y = fmaf(e.a[c * 4 + 2], in[k][2].v[j],
                                     fmaf(e.a[c * 4 + 1], in[k][1].v[j], fmaf(e.a[c * 4], in[k][0].v[j], e.a[c * 4 + 3])));
                r.v[j] = e.on ? y : in[k][c].v[j];
            }
            store4(o[c], p0, P, oa[c], r);
        }
    }
}

// GI: g_image = A^T g_out.  GP: the workgroup's row of the 12 sums of g_params (rows of a passed-through entry are never read
// and are not written).  One pass: g_out (and, with GP, the image) is read once.
template <bool GI, bool GP>
__global__ __launch_bounds__(kThreads) void exposure_bwd_kernel(int V, long long P, int chunks, const float* __restrict__ image,
                                                                const float* __restrict__ params,
                                                                const long long* __restrict__ view_ids,
                                                                const float* __restrict__ g_out, float* __restrict__ g_image,
                                                                double* __restrict__ rows)
{
    // groups loaded per pass: with the sums one (6 waves per SIMD; measured against 2 and 4: DESIGN.md), else all
    constexpr int NB = GP ? 1 : kIters;
    __shared__ double s_red[GP ? kWaves * kGradSums : 1];
    const Entry e = entry_of_block(V, chunks, params, view_ids);
    const bool sums = GP && e.on;
    const float *x[3], *g[3];
    float* o[3];
    bool xa[3], ga[3], oa[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t off = ((size_t)e.b * 3 + c) * (size_t)P;
        x[c] = GP ? image + off : nullptr;
        g[c] = g_out + off;
        o[c] = GI ? g_image + off : nullptr;
        xa[c] = aligned16(x[c]);
        ga[c] = aligned16(g[c]);
        oa[c] = aligned16(o[c]);
    }
    double s[kGradSums];
#pragma unroll
    for (int f = 0; f < kGradSums; ++f) s[f] = 0.0;
    const long long g0 = (long long)e.chunk * kGroups + threadIdx.x;
#pragma unroll
    for (int k0 = 0; k0 < kIters; k0 += NB) {
        Px4 gin[NB][3], xin[NB][3];
#pragma unroll
        for (int k = 0; k < NB; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const long long p0 = (g0 + (k0 + k) * kThreads) * kVec;
                gin[k][c] = load4(g[c], p0, P, ga[c]);
                if (GP) {
                    if (sums) {
                        xin[k][c] = load4(x[c], p0, P, xa[c]);
                    } else {
#pragma unroll
                        for (int j = 0; j < kVec; ++j) xin[k][c].v[j] = 0.0f;
                    }
                }
            }
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const long long p0 = (g0 + (k0 + k) * kThreads) * kVec;
            if (p0 >= P) continue;
            if (GI) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {                               // (c: the channel of the image here)
                    Px4 r;
#pragma unroll
                    for (int j = 0; j < kVec; ++j) {
                        const float y = fmaf(e.a[8 + c], gin[k][2].v[j], fmaf(e.a[4 + c], gin[k][1].v[j], e.a[c] * gin[k][0].v[j]));
                        r.v[j] = e.on ? y : gin[k][c].v[j];
                    }
                    store4(o[c], p0, P, oa[c], r);
                }
            }
            if (sums) {                                                      // (a pixel beyond P was loaded as 0 and adds +0)
#pragma unroll
                for (int j = 0; j < kVec; ++j)
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double gc = (double)gin[k][c].v[j];
#pragma unroll
                        for (int q = 0; q < 3; ++q) s[c * 4 + q] = fma(gc, (double)xin[k][q].v[j], s[c * 4 + q]);
                        s[c * 4 + 3] += gc;
                    }
            }
        }
    }
    if constexpr (GP) {
        block_sum_waves<kGradSums>(s, s_red);
        if (threadIdx.x == 0 && e.on) {
            double* row = rows + (size_t)blockIdx.x * kGradSums;
#pragma unroll
            for (int f = 0; f < kGradSums; ++f) row[f] = s[f];
        }
    }
}

// the rows of view blockIdx.x: entries in index order, an entry's rows strided over the threads, then block_sum_waves.  The
// totals are valid in thread 0.
template <int F>
__device__ __forceinline__ void view_sum(int B, int chunks, const long long* __restrict__ view_ids, const double* __restrict__ rows,
                                         double (&s)[F], double* s_red)
{
    const long long v = blockIdx.x;
#pragma unroll
    for (int f = 0; f < F; ++f) s[f] = 0.0;
    const long long first = view_ids ? 0 : v, last = view_ids ? B : v + 1;      // (no ids: B == V, entry v alone)
    for (long long b = first; b < last; ++b) {
        if (view_ids && view_ids[b] != v) continue;
        const double* r = rows + (size_t)b * chunks * F;
        for (int k = threadIdx.x; k < chunks; k += kThreads)
#pragma unroll
            for (int f = 0; f < F; ++f) s[f] += r[(size_t)k * F + f];
    }
    block_sum_waves<F>(s, s_red);
}

// one workgroup per view: g_params [V,3,4], written in full (exactly 0 for a view without an entry)
__global__ __launch_bounds__(kThreads) void exposure_bwd_finalize_kernel(int B, int chunks, const long long* __restrict__ view_ids,
                                                                         const double* __restrict__ rows,
                                                                         float* __restrict__ g_params)
{
    __shared__ double s_red[kWaves * kGradSums];
    double s[kGradSums];
    view_sum<kGradSums>(B, chunks, view_ids, rows, s, s_red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int f = 0; f < kGradSums; ++f) g_params[(size_t)blockIdx.x * 12 + f] = (float)s[f];
}

// the workgroup's row of the 22 sums of the fit.  pred, target and the mask are read once.
template <bool MASK>
__global__ __launch_bounds__(kThreads) void exposure_fit_kernel(int V, long long P, int chunks, const float* __restrict__ pred,
                                                                const float* __restrict__ target,
                                                                const uint8_t* __restrict__ mask,
                                                                const long long* __restrict__ view_ids, double* __restrict__ rows)
{
    __shared__ double s_red[kWaves * kFitSums];
    const long long b = blockIdx.x / chunks;
    const int chunk = (int)(blockIdx.x - b * chunks);
    const long long id = view_ids ? view_ids[b] : b;
    if (id < 0 || id >= (long long)V) return;                               // (wave-uniform; such rows are never read)
    const float *x[3], *y[3];
    bool xa[3], ya[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const size_t off = ((size_t)b * 3 + c) * (size_t)P;
        x[c] = pred + off;
        y[c] = target + off;
        xa[c] = aligned16(x[c]);
        ya[c] = aligned16(y[c]);
    }
    const uint8_t* m = MASK ? mask + (size_t)b * (size_t)P : nullptr;
    const bool ma = ((uintptr_t)m & 3) == 0;
    double s[kFitSums];
#pragma unroll
    for (int f = 0; f < kFitSums; ++f) s[f] = 0.0;
    const long long g0 = (long long)chunk * kGroups + threadIdx.x;
    // rolled, one group per pass: the 22 fp64 sums already take 44 registers, and the kernel is faster at 4 waves per SIMD
    // (106 registers) than with its loads batched at 2 or 3 (measured: DESIGN.md)
#pragma unroll 1
    for (int k0 = 0; k0 < kIters; ++k0) {
        constexpr int NB = 1;
        Px4 xin[NB][3], yin[NB][3];
        uint32_t min[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const long long p0 = (g0 + (k0 + k) * kThreads) * kVec;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                xin[k][c] = load4(x[c], p0, P, xa[c]);
                yin[k][c] = load4(y[c], p0, P, ya[c]);
            }
            min[k] = MASK ? load_mask4(m, p0, P, ma) : 0xffffffffu;
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const long long p0 = (g0 + (k0 + k) * kThreads) * kVec;
#pragma unroll
            for (int j = 0; j < kVec; ++j) {
                bool ok = p0 + j < P && ((min[k] >> (8 * j)) & 0xffu) != 0;
#pragma unroll
                for (int c = 0; c < 3; ++c) ok = ok && fabsf(xin[k][c].v[j]) < INFINITY && fabsf(yin[k][c].v[j]) < INFINITY;
                // an invalid pixel enters as X = 0, y = 0 and a count of 0: every sum keeps its bits
                double X[3], Y[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    X[c] = ok ? (double)xin[k][c].v[j] : 0.0;
                    Y[c] = ok ? (double)yin[k][c].v[j] : 0.0;
                }
                s[0] = fma(X[0], X[0], s[0]);
                s[1] = fma(X[0], X[1], s[1]);
                s[2] = fma(X[0], X[2], s[2]);
                s[3] += X[0];
                s[4] = fma(X[1], X[1], s[4]);
                s[5] = fma(X[1], X[2], s[5]);
                s[6] += X[1];
                s[7] = fma(X[2], X[2], s[7]);
                s[8] += X[2];
                s[kCnt] += ok ? 1.0 : 0.0;
#pragma unroll
                for (int q = 0; q < 3; ++q)
#pragma unroll
                    for (int c = 0; c < 3; ++c) s[kR + q * 3 + c] = fma(X[q], Y[c], s[kR + q * 3 + c]);
#pragma unroll
                for (int c = 0; c < 3; ++c) s[kR + 9 + c] += Y[c];
            }
        }
    }
    block_sum_waves<kFitSums>(s, s_red);
    if (threadIdx.x == 0) {
        double* row = rows + (size_t)blockIdx.x * kFitSums;
#pragma unroll
        for (int f = 0; f < kFitSums; ++f) row[f] = s[f];
    }
}

// one workgroup per view: the view's 22 sums, then (thread 0) the ridge-regularised normal equations by Cholesky in fp64
__global__ __launch_bounds__(kThreads) void exposure_fit_finalize_kernel(int B, int chunks, const long long* __restrict__ view_ids,
                                                                         const double* __restrict__ rows, double ridge,
                                                                         float* __restrict__ params, long long* __restrict__ count,
                                                                         uint8_t* __restrict__ solved)
{
    __shared__ double s_red[kWaves * kFitSums];
    double s[kFitSums];
    view_sum<kFitSums>(B, chunks, view_ids, rows, s, s_red);
    if (threadIdx.x != 0) return;
    const double cnt = s[kCnt], lam = ridge * cnt;
    double M[4][4] = {{s[0], s[1], s[2], s[3]}, {s[1], s[4], s[5], s[6]}, {s[2], s[5], s[7], s[8]}, {s[3], s[6], s[8], s[9]}};
    double rhs[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        M[k][k] += lam;
#pragma unroll
        for (int c = 0; c < 3; ++c) rhs[k][c] = s[kR + k * 3 + c] + (k == c ? lam : 0.0);
    }
    bool ok = cnt > 0.0;
    double L[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double d = M[j][j];
#pragma unroll
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
        ok = ok && d > 0.0 && d < (double)INFINITY;
        L[j][j] = sqrt(d);
#pragma unroll
        for (int i = j + 1; i < 4; ++i) {
            double a = M[i][j];
#pragma unroll
            for (int k = 0; k < j; ++k) a -= L[i][k] * L[j][k];
            L[i][j] = a / L[j][j];
        }
    }
    float* out = params + (size_t)blockIdx.x * 12;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double z[4], p[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            double a = rhs[i][c];
#pragma unroll
            for (int k = 0; k < i; ++k) a -= L[i][k] * z[k];
            z[i] = a / L[i][i];
        }
#pragma unroll
        for (int i = 3; i >= 0; --i) {
            double a = z[i];
#pragma unroll
            for (int k = i + 1; k < 4; ++k) a -= L[k][i] * p[k];
            p[i] = a / L[i][i];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) out[c * 4 + k] = ok ? (float)p[k] : (k == c ? 1.0f : 0.0f);
    }
    count[blockIdx.x] = (long long)cnt;
    solved[blockIdx.x] = ok ? 1 : 0;
}

struct Grid {
    long long P;
    int chunks;
    unsigned blocks;
};

// FS_OK, or why the sizes cannot run
int make_grid(int32_t B, int32_t H, int32_t W, Grid& g)
{
    if (B <= 0 || H <= 0 || W <= 0) return FS_ERR_INVALID_ARG;
    g.P = (long long)H * W;
    if (g.P > 0x7fffffffLL) return FS_ERR_UNSUPPORTED;
    g.chunks = (int)((g.P + kChunk - 1) / kChunk);
    const long long blocks = (long long)B * g.chunks;
    if (blocks > 0x7fffffffLL) return FS_ERR_UNSUPPORTED;
    g.blocks = (unsigned)blocks;
    return FS_OK;
}

}  // namespace

}  // namespace fs

using namespace fs;

FS_API int fs_exposure_api_version(void) { return FS_EXPOSURE_API_VERSION; }

FS_API size_t fs_exposure_scratch_bytes(int32_t B, int32_t H, int32_t W)
{
    Grid g;
    if (make_grid(B, H, W, g) != FS_OK) return 0;
    return align_up((size_t)g.blocks * kFitSums * sizeof(double), 256);
}

FS_API int fs_exposure_apply_forward(int32_t B, int32_t V, int32_t H, int32_t W, const float* image, const float* params,
                                     const int64_t* view_ids, float* out, void* stream_)
{
    Grid g;
    if (V <= 0 || !image || !params || !out || (!view_ids && B != V)) return FS_ERR_INVALID_ARG;
    if (const int st = make_grid(B, H, W, g)) return st;
    hipLaunchKernelGGL(exposure_fwd_kernel, dim3(g.blocks), dim3(kThreads), 0, (hipStream_t)stream_, V, g.P, g.chunks, image,
                       params, (const long long*)view_ids, out);
    FS_CHECK_LAUNCH("exposure_apply_forward");
    return FS_OK;
}

FS_API int fs_exposure_apply_backward(int32_t B, int32_t V, int32_t H, int32_t W, const float* image, const float* params,
                                      const int64_t* view_ids, const float* g_out, float* g_image, float* g_params, void* scratch,
                                      void* stream_)
{
    Grid g;
    if (V <= 0 || !params || !g_out || (!g_image && !g_params) || (g_params && (!image || !scratch)) || (!view_ids && B != V))
        return FS_ERR_INVALID_ARG;
    if (const int st = make_grid(B, H, W, g)) return st;
    hipStream_t st = (hipStream_t)stream_;
    const long long* ids = (const long long*)view_ids;
    double* rows = static_cast<double*>(scratch);
    const dim3 grid(g.blocks), block(kThreads);
    if (g_image && g_params)
        hipLaunchKernelGGL((exposure_bwd_kernel<true, true>), grid, block, 0, st, V, g.P, g.chunks, image, params, ids, g_out, g_image, rows);
    else if (g_image)
        hipLaunchKernelGGL((exposure_bwd_kernel<true, false>), grid, block, 0, st, V, g.P, g.chunks, image, params, ids, g_out, g_image,
                           rows);
    else
        hipLaunchKernelGGL((exposure_bwd_kernel<false, true>), grid, block, 0, st, V, g.P, g.chunks, image, params, ids, g_out, g_image,
                           rows);
    if (g_params)
        hipLaunchKernelGGL(exposure_bwd_finalize_kernel, dim3((unsigned)V), block, 0, st, B, g.chunks, ids, (const double*)rows, g_params);
    FS_CHECK_LAUNCH("exposure_apply_backward");
    return FS_OK;
}

FS_API int fs_exposure_fit(int32_t B, int32_t V, int32_t H, int32_t W, const float* pred, const float* target, const uint8_t* mask,
                           const int64_t* view_ids, double ridge, float* params, int64_t* count, uint8_t* solved, void* scratch,
                           void* stream_)
{
    Grid g;
    if (V <= 0 || !pred || !target || !params || !count || !solved || !scratch || (!view_ids && B != V) ||
        !(ridge >= 0.0 && ridge < (double)INFINITY))
        return FS_ERR_INVALID_ARG;
    if (const int st = make_grid(B, H, W, g)) return st;
    hipStream_t st = (hipStream_t)stream_;
    const long long* ids = (const long long*)view_ids;
    double* rows = static_cast<double*>(scratch);
    const dim3 grid(g.blocks), block(kThreads);
    if (mask)
        hipLaunchKernelGGL((exposure_fit_kernel<true>), grid, block, 0, st, V, g.P, g.chunks, pred, target, mask, ids, rows);
    else
        hipLaunchKernelGGL((exposure_fit_kernel<false>), grid, block, 0, st, V, g.P, g.chunks, pred, target, mask, ids, rows);
    hipLaunchKernelGGL(exposure_fit_finalize_kernel, dim3((unsigned)V), block, 0, st, B, g.chunks, ids, (const double*)rows, ridge, params,
                       (long long*)count, solved);
    FS_CHECK_LAUNCH("exposure_fit");
    return FS_OK;
}
