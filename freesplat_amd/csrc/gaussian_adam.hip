// gaussian_adam.hip -- fused Adam step over the parameters of one scene's Gaussians (include/freesplat_amd_optim.h).
//
// One launch covers the five arrays (means, log-scales, rotations, opacity logits, SH).  Each array is a flat run of floats
// cut into chunks of kChunk = 1024; the chunks of all arrays are numbered in one sequence (the by-value segment table holds
// every array's first and last chunk number), workgroup b takes chunks b, b + grid, b + 2 grid, ... and walks the arrays in
// order, so the array -- and with it the activation and the row width -- is a compile-time constant inside each loop.  A lane
// owns 4 consecutive floats: one 16-byte load of p, g, exp_avg, exp_avg_sq and one 16-byte store of p, exp_avg, exp_avg_sq (and
// of the activated output) where the array's pointers are 16-byte aligned and the 4 floats exist, 4-byte accesses otherwise
// (the tail of an array, or an unaligned array).  28 bytes per parameter, read and written once.
//
// A 16-byte group may straddle rows (row widths 3, 27, ...): the visibility of a row and the sh_dc / sh_rest split are decided
// per element.  A group with no visible element loads and stores nothing; a group with some stores its visible elements one
// by one, so that nothing of an invisible row is written.
//
// Numerics: fp32 per element, every operation rounded on its own (the translation unit is compiled with -ffp-contract=off).
// The bias corrections 1 - beta^t are formed in double precision by one lane per workgroup from the device-resident step
// counter (in fp32, 1 - 0.999^t at small t loses four digits) and handed to the workgroup through LDS as the six step
// sizes lr / bc1 and sqrt(bc2).  No atomics: the same bits on every run and stream.
#include "fs_common.h"

#include <math.h>

#include "../../include/freesplat_amd_optim.h"
#include "gaussian_act.h"

namespace fs {

namespace {

constexpr int kAdamThreads = 256;
constexpr int kVec = 4;                                      // floats per lane and iteration: one 16-byte access
constexpr uint32_t kChunk = kAdamThreads * kVec;             // floats of one array a workgroup handles per iteration
constexpr uint32_t kMaxGrid = 2048;                          // 8 workgroups per CU; the rest is grid-strided

// The activations act_scale / act_opacity (gaussian_act.h): the step (before the update, for the chain rule; after it, for
// the outputs) and fs_gaussian_activate call these two, so one raw value gives one bit pattern everywhere.

struct Segment {
    float* p;
    const float* g;
    float* m;
    float* v;
    float* act;              // activated output of the array (scales, opacities), else NULL
    uint32_t len;            // floats
    uint32_t first_chunk;    // chunk numbers [first_chunk, end_chunk) of the launch belong to this array
    uint32_t end_chunk;
    uint32_t vec;            // every pointer above is 16-byte aligned
};

struct StepArgs {
    Segment seg[FS_OPTIM_ARRAYS];
    const int32_t* visible;
    const float* lr;
    const int32_t* step;
    double beta1, beta2;
    float b1, omb1, b2, omb2, eps;     // omb = 1 - beta, rounded once from the double
    int32_t M;
};

struct Hyper {
    float b1, omb1, b2, omb2, eps, sqrt_bc2;
};

// base^e by squaring: at most 31 products in double precision, no library call
__device__ __forceinline__ double ipow(double base, uint32_t e)
{
    double r = 1.0;
    while (e) {
        if (e & 1u) r *= base;
        base *= base;
        e >>= 1;
    }
    return r;
}

// row_width<KIND>(M), row_of<KIND>(i, M, q, r): gaussian_act.h

// One element.  g arrives as the gradient with respect to the activated value; `act` receives the activation of the new
// raw value (scales, opacities).
template <int KIND>
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, float step_size, const Hyper& h, float& act)
{
    if constexpr (KIND == FS_OPTIM_SCALES) g = g * act_scale(p);
    if constexpr (KIND == FS_OPTIM_OPACITIES) {
        const float o = act_opacity(p);
        g = g * o * (1.0f - o);
    }
    m = h.b1 * m + h.omb1 * g;
    v = h.b2 * v + h.omb2 * g * g;
    const float denom = sqrtf(v) / h.sqrt_bc2 + h.eps;
    p = p - step_size * (m / denom);
    if constexpr (KIND == FS_OPTIM_SCALES) act = act_scale(p);
    if constexpr (KIND == FS_OPTIM_OPACITIES) act = act_opacity(p);
}

template <int KIND, bool SPARSE>
__device__ __forceinline__ void run_segment(const StepArgs& a, const Hyper& h, const float* s_step, uint32_t& chunk)
{
    constexpr bool kHasAct = KIND == FS_OPTIM_SCALES || KIND == FS_OPTIM_OPACITIES;
    constexpr int kGroup = KIND == FS_OPTIM_MEANS ? FS_OPTIM_LR_MEANS : KIND == FS_OPTIM_SCALES ? FS_OPTIM_LR_SCALES
                         : KIND == FS_OPTIM_ROTATIONS ? FS_OPTIM_LR_ROTATIONS : KIND == FS_OPTIM_OPACITIES ? FS_OPTIM_LR_OPACITIES
                         : FS_OPTIM_LR_SH_DC;
    const Segment& s = a.seg[KIND];
    const uint32_t width = row_width<KIND>(a.M);
    for (; chunk < s.end_chunk; chunk += gridDim.x) {
        const uint32_t i0 = (chunk - s.first_chunk) * kChunk + threadIdx.x * kVec;
        if (i0 >= s.len) continue;
        const uint32_t n = s.len - i0 < (uint32_t)kVec ? s.len - i0 : (uint32_t)kVec;
        uint32_t row0 = 0, rem0 = 0;
        if constexpr (SPARSE || KIND == FS_OPTIM_SHS) row_of<KIND>(i0, a.M, row0, rem0);
        bool on[kVec];
        float ss[kVec];
        bool any = false, all = true;
#pragma unroll
        for (int j = 0; j < kVec; ++j) {
            uint32_t row = row0, r = rem0 + j;
            if constexpr (KIND == FS_OPTIM_OPACITIES) {
                row = row0 + j; r = 0;
            } else if (r >= width) {           // i0 is a multiple of 4 and width is 3, 4 or >= 12: one wrap at the most
                r -= width; ++row;
            }
            on[j] = (uint32_t)j < n;
            if constexpr (SPARSE) {
                if (on[j]) on[j] = a.visible[row] > 0;
            }
            ss[j] = KIND == FS_OPTIM_SHS ? (r < 3u ? s_step[FS_OPTIM_LR_SH_DC] : s_step[FS_OPTIM_LR_SH_REST]) : s_step[kGroup];
            any = any || on[j];
            all = all && on[j];
        }
        if (!any) continue;
        if (s.vec && n == (uint32_t)kVec) {
            const float4 p4 = *reinterpret_cast<const float4*>(s.p + i0), g4 = *reinterpret_cast<const float4*>(s.g + i0);
            const float4 m4 = *reinterpret_cast<const float4*>(s.m + i0), v4 = *reinterpret_cast<const float4*>(s.v + i0);
            float p[kVec] = {p4.x, p4.y, p4.z, p4.w}, m[kVec] = {m4.x, m4.y, m4.z, m4.w}, v[kVec] = {v4.x, v4.y, v4.z, v4.w};
            const float g[kVec] = {g4.x, g4.y, g4.z, g4.w};
            float act[kVec] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < kVec; ++j)
                if (on[j]) adam_element<KIND>(p[j], g[j], m[j], v[j], ss[j], h, act[j]);
            if (all) {
                *reinterpret_cast<float4*>(s.p + i0) = make_float4(p[0], p[1], p[2], p[3]);
                *reinterpret_cast<float4*>(s.m + i0) = make_float4(m[0], m[1], m[2], m[3]);
                *reinterpret_cast<float4*>(s.v + i0) = make_float4(v[0], v[1], v[2], v[3]);
                if constexpr (kHasAct) *reinterpret_cast<float4*>(s.act + i0) = make_float4(act[0], act[1], act[2], act[3]);
            } else {
#pragma unroll
                for (int j = 0; j < kVec; ++j)
                    if (on[j]) {
                        s.p[i0 + j] = p[j]; s.m[i0 + j] = m[j]; s.v[i0 + j] = v[j];
                        if constexpr (kHasAct) s.act[i0 + j] = act[j];
                    }
            }
        } else {
#pragma unroll
            for (int j = 0; j < kVec; ++j)
                if (on[j]) {
                    float p = s.p[i0 + j], m = s.m[i0 + j], v = s.v[i0 + j], act = 0.0f;
                    adam_element<KIND>(p, s.g[i0 + j], m, v, ss[j], h, act);
                    s.p[i0 + j] = p; s.m[i0 + j] = m; s.v[i0 + j] = v;
                    if constexpr (kHasAct) s.act[i0 + j] = act;
                }
        }
    }
}

template <bool SPARSE>
__global__ __launch_bounds__(kAdamThreads, 8) void gaussian_adam_step_kernel(const StepArgs a)
{
    __shared__ float s_step[FS_OPTIM_LR_GROUPS + 2];         // lr / bc1 per group, sqrt(bc2)
    if (threadIdx.x == 0) {
        const uint32_t t = (uint32_t)a.step[0] + 1u;
        const double bc1 = 1.0 - ipow(a.beta1, t), bc2 = 1.0 - ipow(a.beta2, t);
#pragma unroll
        for (int k = 0; k < FS_OPTIM_LR_GROUPS; ++k) s_step[k] = (float)((double)a.lr[k] / bc1);
        s_step[FS_OPTIM_LR_GROUPS] = (float)sqrt(bc2);
    }
    __syncthreads();
    Hyper h;
    h.b1 = a.b1; h.omb1 = a.omb1; h.b2 = a.b2; h.omb2 = a.omb2; h.eps = a.eps;
    h.sqrt_bc2 = s_step[FS_OPTIM_LR_GROUPS];
    uint32_t chunk = blockIdx.x;
    run_segment<FS_OPTIM_MEANS, SPARSE>(a, h, s_step, chunk);
    run_segment<FS_OPTIM_SCALES, SPARSE>(a, h, s_step, chunk);
    run_segment<FS_OPTIM_ROTATIONS, SPARSE>(a, h, s_step, chunk);
    run_segment<FS_OPTIM_OPACITIES, SPARSE>(a, h, s_step, chunk);
    run_segment<FS_OPTIM_SHS, SPARSE>(a, h, s_step, chunk);
}

// launched after the step kernel on the same stream: the counter the next step reads as t - 1
__global__ void gaussian_adam_advance_kernel(int32_t* step) { step[0] = step[0] + 1; }

__global__ __launch_bounds__(kAdamThreads) void gaussian_activate_kernel(size_t n_scales, size_t n_total,
                                                                         const float* __restrict__ log_scales,
                                                                         const float* __restrict__ logits,
                                                                         float* __restrict__ out_scales,
                                                                         float* __restrict__ out_opacities)
{
    for (size_t i = (size_t)blockIdx.x * kAdamThreads + threadIdx.x; i < n_total; i += (size_t)gridDim.x * kAdamThreads) {
        if (i < n_scales)
            out_scales[i] = act_scale(log_scales[i]);
        else
            out_opacities[i - n_scales] = act_opacity(logits[i - n_scales]);
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

}  // namespace fs

using namespace fs;

FS_API int fs_optim_api_version(void) { return FS_OPTIM_API_VERSION; }

FS_API int fs_gaussian_activate(int32_t N, const float* log_scales, const float* logits, float* out_scales, float* out_opacities,
                                void* stream_)
{
    if (N < 0) return FS_ERR_INVALID_ARG;
    if (N == 0) return FS_OK;
    if (!log_scales || !logits || !out_scales || !out_opacities) return FS_ERR_INVALID_ARG;
    const size_t n_scales = 3 * (size_t)N, n_total = 4 * (size_t)N;
    const size_t blocks = (n_total + kAdamThreads - 1) / kAdamThreads;
    const dim3 grid((unsigned)(blocks < kMaxGrid ? blocks : kMaxGrid));
    hipLaunchKernelGGL(gaussian_activate_kernel, grid, dim3(kAdamThreads), 0, (hipStream_t)stream_, n_scales, n_total, log_scales,
                       logits, out_scales, out_opacities);
    FS_CHECK_LAUNCH("gaussian_activate");
    return FS_OK;
}

FS_API int fs_gaussian_adam_step(int32_t N, int32_t M, float* const* p, const float* const* g, float* const* exp_avg,
                                 float* const* exp_avg_sq, const int32_t* visible, const float* lr_dev, int32_t* step_dev,
                                 double beta1, double beta2, double eps, float* out_scales, float* out_opacities, void* stream_)
{
    if (N < 0 || (M != 1 && M != 4 && M != 9 && M != 16)) return FS_ERR_INVALID_ARG;
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0)) return FS_ERR_INVALID_ARG;
    if (3ll * M * N > 0x7FFFFFFFll) return FS_ERR_INVALID_ARG;
    if (N == 0) return FS_OK;
    if (!p || !g || !exp_avg || !exp_avg_sq || !lr_dev || !step_dev || !out_scales || !out_opacities) return FS_ERR_INVALID_ARG;
    bool any_g = false;
    for (int k = 0; k < FS_OPTIM_ARRAYS; ++k) {
        if (!p[k] || !exp_avg[k] || !exp_avg_sq[k]) return FS_ERR_INVALID_ARG;
        any_g = any_g || g[k];
    }
    if (!any_g) return FS_ERR_INVALID_ARG;

    const uint32_t widths[FS_OPTIM_ARRAYS] = {3u, 3u, 4u, 1u, 3u * (uint32_t)M};
    StepArgs a;
    uint32_t chunks = 0;
    for (int k = 0; k < FS_OPTIM_ARRAYS; ++k) {
        Segment& s = a.seg[k];
        s.p = p[k]; s.g = g[k]; s.m = exp_avg[k]; s.v = exp_avg_sq[k];
        s.act = k == FS_OPTIM_SCALES ? out_scales : k == FS_OPTIM_OPACITIES ? out_opacities : nullptr;
        s.len = widths[k] * (uint32_t)N;
        s.first_chunk = chunks;
        if (g[k]) chunks += (s.len + kChunk - 1) / kChunk;       // no gradient: no chunks, the array is not touched
        s.end_chunk = chunks;
        s.vec = aligned16(s.p) && aligned16(s.g) && aligned16(s.m) && aligned16(s.v) && aligned16(s.act);
    }
    a.visible = visible;
    a.lr = lr_dev;
    a.step = step_dev;
    a.beta1 = beta1; a.beta2 = beta2;
    a.b1 = (float)beta1; a.omb1 = (float)(1.0 - beta1);
    a.b2 = (float)beta2; a.omb2 = (float)(1.0 - beta2);
    a.eps = (float)eps;
    a.M = M;
    hipStream_t st = (hipStream_t)stream_;
    const dim3 grid(chunks < kMaxGrid ? chunks : kMaxGrid);
    if (visible)
        hipLaunchKernelGGL(gaussian_adam_step_kernel<true>, grid, dim3(kAdamThreads), 0, st, a);
    else
        hipLaunchKernelGGL(gaussian_adam_step_kernel<false>, grid, dim3(kAdamThreads), 0, st, a);
    hipLaunchKernelGGL(gaussian_adam_advance_kernel, dim3(1), dim3(1), 0, st, step_dev);
    FS_CHECK_LAUNCH("gaussian_adam_step");
    return FS_OK;
}
