// gaussian_density.hip -- adaptive density control for the Gaussians of one scene: clone, split, prune
// (include/freesplat_amd_density.h; freesplat_amd.refine.GaussianAdam.accumulate / densify / reset_opacity).
//
//   accumulate     one elementwise launch over the view-space gradient norms of the visible rows.
//   plan           three launches, a compaction on fs_scan.h's helpers: every workgroup classifies kScanBlock = 1024 source rows
//                  (256 threads x 4) and counts their output rows; ONE workgroup scans the block sums (a thread takes a
//                  contiguous slice of them, so any number of blocks is covered); every workgroup scans its own rows and
//                  scatters offset[] and the output -> source map src[].  Integer arithmetic only, apart from the single fp32
//                  product grad_threshold * denom; no workgroup waits on another.
//   apply          the hot path, one launch driven by the OUTPUT: the destination arrays are flat runs of floats cut into
//                  chunks of 1024 numbered in one sequence, as in gaussian_adam.hip; a lane owns 4 consecutive destination
//                  floats and finds their source through src[] alone (source row, first / second output, split flag).  Rows of a multiple of 16 bytes (rotations, SH with M = 4 or
//                  16 -- 52 of the 59 floats at SH degree 3) keep their alignment under any compaction: 16-byte loads and
//                  stores.  The other arrays (widths 3, 1, 27) are shifted by an arbitrary number of floats: 4-byte loads
//                  (neighbouring lanes read neighbouring addresses, the reads are monotone in the source) and 16-byte stores.
//                  Moments are read only where they survive (kept rows, clone originals) and written as zeros elsewhere.
//   reset_opacity  one elementwise launch.
//
// Numerics: fp32, every operation rounded on its own (-ffp-contract=off).  No float atomics: the same bits on every run and
// stream.
#include "fs_common.h"

#include <math.h>

#include "../../include/freesplat_amd_density.h"
#include "fs_reduce.h"
#include "fs_scan.h"
#include "gaussian_act.h"

namespace fs {

namespace {

constexpr int kThreads = 256;
constexpr int kVec = 4;
constexpr uint32_t kScanBlock = kThreads * kVec;             // source rows per plan workgroup
constexpr uint32_t kChunk = kThreads * kVec;                 // destination floats per apply workgroup and iteration
constexpr uint32_t kMaxGrid = 2048;                          // 8 workgroups per CU; the rest is grid-strided
constexpr float kLogSplit = 0.47000363f;                     // logf(1.6f)
constexpr uint32_t kSplitTag = 0x80000000u;                  // src[o] = (2 i + j) | kSplitTag for the children of a split row

// ---------------------------------------------------------------------------------------------------------- accumulate

__global__ __launch_bounds__(kThreads) void density_accumulate_kernel(uint32_t N, const float* __restrict__ g,
                                                                      const int32_t* __restrict__ radii,
                                                                      float* __restrict__ grad_accum, float* __restrict__ denom,
                                                                      float* __restrict__ max_radii)
{
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < N; i += gridDim.x * kThreads) {
        const int32_t r = radii[i];
        if (r <= 0) continue;
        const float gx = g[3 * (size_t)i], gy = g[3 * (size_t)i + 1];
        grad_accum[i] = grad_accum[i] + sqrtf(gx * gx + gy * gy);
        denom[i] = denom[i] + 1.0f;
        max_radii[i] = fmaxf(max_radii[i], (float)r);
    }
}

// ---------------------------------------------------------------------------------------------------------------- plan

struct PlanArgs {
    const float* grad_accum;
    const float* denom;
    const float* max_radii;
    const float* scales;
    const float* opacities;
    float grad_threshold, dense_scale, min_opacity, max_screen_size, prune_scale, child_prune_scale;
    uint32_t N, nb;
};

__device__ __forceinline__ uint32_t classify(const PlanArgs& a, uint32_t i)
{
    const float* sc = a.scales + 3 * (size_t)i;
    const float s_max = fmaxf(fmaxf(sc[0], sc[1]), sc[2]);
    const float d = a.denom[i];
    const bool hot = d > 0.0f && a.grad_accum[i] >= a.grad_threshold * d;
    const bool split = hot && s_max > a.dense_scale;
    bool drop = a.opacities[i] < a.min_opacity;
    if (!split && a.max_screen_size > 0.0f) drop = drop || a.max_radii[i] > a.max_screen_size;
    if (a.prune_scale > 0.0f) drop = drop || s_max > (split ? a.child_prune_scale : a.prune_scale);
    return drop ? FS_DENSITY_DROPPED : split ? FS_DENSITY_SPLIT : hot ? FS_DENSITY_CLONE : FS_DENSITY_KEPT;
}

__device__ __forceinline__ uint32_t outputs_of(uint32_t kind) { return kind == FS_DENSITY_DROPPED ? 0u : kind == FS_DENSITY_KEPT ? 1u : 2u; }

// block_counts: four runs of nb uint32 -- output rows, clones, splits, drops of each workgroup's 1024 source rows
__global__ __launch_bounds__(kThreads) void density_count_kernel(const PlanArgs a, uint8_t* __restrict__ kind,
                                                                 uint32_t* __restrict__ block_counts)
{
    __shared__ unsigned long long s_w[kThreads / kWave];
    const uint32_t base = blockIdx.x * kScanBlock + threadIdx.x * kVec;
    uint32_t packed = 0;
    unsigned long long c = 0;                                // four 16-bit counters: a workgroup emits at most 2048 rows
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        if (base + k >= a.N) break;
        const uint32_t kd = classify(a, base + k);
        packed |= kd << (8u * k);
        c += (unsigned long long)outputs_of(kd) | ((unsigned long long)(kd == FS_DENSITY_CLONE) << 16) |
             ((unsigned long long)(kd == FS_DENSITY_SPLIT) << 32) | ((unsigned long long)(kd == FS_DENSITY_DROPPED) << 48);
    }
    store_flags4(kind, base, a.N, packed);
    c = wave_sum<unsigned long long>(c);
    if ((threadIdx.x & (kWave - 1)) == 0) s_w[threadIdx.x / kWave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long t = waves_total<unsigned long long>(s_w, 1);
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) block_counts[q * a.nb + blockIdx.x] = (uint32_t)(t >> (16u * q)) & 0xFFFFu;
    }
}

// One workgroup: exclusive scan of run 0 in place, sums of all four runs into totals (fs_scan.h's slice_scan).
__global__ __launch_bounds__(kScanThreads) void density_scan_blocks_kernel(uint32_t nb, uint32_t* __restrict__ block_counts,
                                                                           int32_t* __restrict__ totals)
{
    __shared__ uint32_t part[kScanThreads];
    for (uint32_t q = 0; q < 4; ++q) {
        uint32_t* a = block_counts + (size_t)q * nb;
        const uint32_t total = slice_scan<uint32_t>(a, nb, q == 0 ? a : nullptr, part);
        if (threadIdx.x == kScanThreads - 1) totals[q] = (int32_t)total;
    }
}

__global__ __launch_bounds__(kThreads) void density_emit_kernel(uint32_t N, const uint8_t* __restrict__ kind,
                                                                const uint32_t* __restrict__ block_offsets,
                                                                uint32_t* __restrict__ offset, uint32_t* __restrict__ src)
{
    __shared__ uint32_t s_w[kThreads / kWave];
    const uint32_t base = blockIdx.x * kScanBlock + threadIdx.x * kVec;
    const uint32_t v = load_flags4(kind, base, N);           // rows past N: dropped, no outputs
    uint32_t cnt[4], c = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        cnt[k] = outputs_of((v >> (8u * k)) & 0xFFu);
        c += cnt[k];
    }
    uint32_t rank = block_offsets[blockIdx.x] + block_excl_scan(c, s_w);
    uint32_t off[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t i = base + k;
        off[k] = rank;
        if (i < N) {
            const uint32_t tag = ((v >> (8u * k)) & 0xFFu) == FS_DENSITY_SPLIT ? kSplitTag : 0u;   // the apply reads src[] only
            if (cnt[k] >= 1u) src[rank] = (2u * i) | tag;
            if (cnt[k] == 2u) src[rank + 1u] = (2u * i + 1u) | tag;
        }
        rank += cnt[k];
    }
    if (base + 3u < N && aligned16(offset + base)) {
        *reinterpret_cast<uint4*>(offset + base) = make_uint4(off[0], off[1], off[2], off[3]);
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            if (base + k < N) offset[base + k] = off[k];
    }
}

// --------------------------------------------------------------------------------------------------------------- apply

struct ApplySeg {
    const float* ps;         // source: parameters, exp_avg, exp_avg_sq
    const float* ms;
    const float* vs;
    float* pd;               // destination
    float* md;
    float* vd;
    float* act;              // activated output of the array (scales, opacities), else NULL
    uint32_t len;            // destination floats
    uint32_t first_chunk;    // chunk numbers [first_chunk, end_chunk) of the launch belong to this array
    uint32_t end_chunk;
    uint32_t vec_dst;        // pd, md, vd, act are 16-byte aligned
    uint32_t vec_src;        // ps, ms, vs are 16-byte aligned
};

struct ApplyArgs {
    ApplySeg seg[FS_OPTIM_ARRAYS];
    const uint32_t* src;
    uint32_t N, seed;
    int32_t M;
};

// component c of R(q / |q|) (s * z) for child `child` of source row i: what a split adds to the parent's mean
__device__ __forceinline__ float split_offset(const ApplyArgs& a, uint32_t i, uint32_t child, uint32_t c)
{
    const float* ls = a.seg[FS_OPTIM_SCALES].ps + 3u * i;
    const float* q = a.seg[FS_OPTIM_ROTATIONS].ps + 4u * i;
    const float row[7] = {act_scale(ls[0]), act_scale(ls[1]), act_scale(ls[2]), q[0], q[1], q[2], q[3]};
    const ScaleRot sr = scale_rot_setup(row);
    const float t0 = sr.s[0] * density_normal(a.seed, i, child, 0u);
    const float t1 = sr.s[1] * density_normal(a.seed, i, child, 1u);
    const float t2 = sr.s[2] * density_normal(a.seed, i, child, 2u);
    const float r0 = c == 0u ? sr.R[0][0] : c == 1u ? sr.R[1][0] : sr.R[2][0];
    const float r1 = c == 0u ? sr.R[0][1] : c == 1u ? sr.R[1][1] : sr.R[2][1];
    const float r2 = c == 0u ? sr.R[0][2] : c == 1u ? sr.R[1][2] : sr.R[2][2];
    return (r0 * t0 + r1 * t1) + r2 * t2;
}

// the moments of a source row survive in its first output unless the row is split
__device__ __forceinline__ bool keeps_moments(uint32_t e) { return (e & (kSplitTag | 1u)) == 0u; }
__device__ __forceinline__ uint32_t source_row(uint32_t e) { return (e & ~kSplitTag) >> 1; }

template <int KIND>
__device__ __forceinline__ void run_segment(const ApplyArgs& a, uint32_t& chunk)
{
    constexpr bool kHasAct = KIND == FS_OPTIM_SCALES || KIND == FS_OPTIM_OPACITIES;
    const ApplySeg& s = a.seg[KIND];
    const uint32_t width = row_width<KIND>(a.M);
    for (; chunk < s.end_chunk; chunk += gridDim.x) {
        const uint32_t i0 = (chunk - s.first_chunk) * kChunk + threadIdx.x * kVec;
        if (i0 >= s.len) continue;
        const uint32_t n = s.len - i0 < (uint32_t)kVec ? s.len - i0 : (uint32_t)kVec;
        uint32_t row0, rem0;
        row_of<KIND>(i0, a.M, row0, rem0);
        if constexpr (KIND == FS_OPTIM_ROTATIONS || KIND == FS_OPTIM_SHS) {
            // a row of a multiple of 4 floats: the group lies inside one row (len is a multiple of 4: n == 4) and its source
            // is as aligned as the source array
            if ((width & 3u) == 0u && s.vec_dst && s.vec_src) {
                const uint32_t e = a.src[row0], i = source_row(e);
                float4 p4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), m4 = p4, v4 = p4;
                if (i < a.N) {
                    const uint32_t at = i * width + rem0;
                    p4 = *reinterpret_cast<const float4*>(s.ps + at);
                    if (keeps_moments(e)) {
                        m4 = *reinterpret_cast<const float4*>(s.ms + at);
                        v4 = *reinterpret_cast<const float4*>(s.vs + at);
                    }
                }
                *reinterpret_cast<float4*>(s.pd + i0) = p4;
                *reinterpret_cast<float4*>(s.md + i0) = m4;
                *reinterpret_cast<float4*>(s.vd + i0) = v4;
                continue;
            }
        }
        float p[kVec] = {0.0f, 0.0f, 0.0f, 0.0f}, m[kVec] = {0.0f, 0.0f, 0.0f, 0.0f}, v[kVec] = {0.0f, 0.0f, 0.0f, 0.0f};
        float act[kVec] = {0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t cur = 0xFFFFFFFFu, e = 0;
#pragma unroll
        for (int j = 0; j < kVec; ++j) {
            if ((uint32_t)j >= n) break;
            uint32_t row = row0, r = rem0 + j;
            if constexpr (KIND == FS_OPTIM_OPACITIES) {
                row = row0 + j; r = 0;
            } else if (r >= width) {           // i0 is a multiple of 4 and width is 3, 4 or >= 12: one wrap at the most
                r -= width; ++row;
            }
            if (row != cur) {
                cur = row;
                e = a.src[row];
            }
            const uint32_t i = source_row(e);
            if (i < a.N) {
                const uint32_t at = i * width + r;
                p[j] = s.ps[at];
                if (keeps_moments(e)) { m[j] = s.ms[at]; v[j] = s.vs[at]; }
                if (e & kSplitTag) {
                    if constexpr (KIND == FS_OPTIM_SCALES) p[j] = p[j] - kLogSplit;
                    if constexpr (KIND == FS_OPTIM_MEANS) p[j] = p[j] + split_offset(a, i, e & 1u, r);
                }
            }
            if constexpr (KIND == FS_OPTIM_SCALES) act[j] = act_scale(p[j]);
            if constexpr (KIND == FS_OPTIM_OPACITIES) act[j] = act_opacity(p[j]);
        }
        if (s.vec_dst && n == (uint32_t)kVec) {
            *reinterpret_cast<float4*>(s.pd + i0) = make_float4(p[0], p[1], p[2], p[3]);
            *reinterpret_cast<float4*>(s.md + i0) = make_float4(m[0], m[1], m[2], m[3]);
            *reinterpret_cast<float4*>(s.vd + i0) = make_float4(v[0], v[1], v[2], v[3]);
            if constexpr (kHasAct) *reinterpret_cast<float4*>(s.act + i0) = make_float4(act[0], act[1], act[2], act[3]);
        } else {
#pragma unroll
            for (int j = 0; j < kVec; ++j)
                if ((uint32_t)j < n) {
                    s.pd[i0 + j] = p[j]; s.md[i0 + j] = m[j]; s.vd[i0 + j] = v[j];
                    if constexpr (kHasAct) s.act[i0 + j] = act[j];
                }
        }
    }
}

__global__ __launch_bounds__(kThreads, 8) void density_apply_kernel(const ApplyArgs a)
{
    uint32_t chunk = blockIdx.x;
    run_segment<FS_OPTIM_MEANS>(a, chunk);
    run_segment<FS_OPTIM_SCALES>(a, chunk);
    run_segment<FS_OPTIM_ROTATIONS>(a, chunk);
    run_segment<FS_OPTIM_OPACITIES>(a, chunk);
    run_segment<FS_OPTIM_SHS>(a, chunk);
}

// ------------------------------------------------------------------------------------------------------- reset_opacity

__global__ __launch_bounds__(kThreads) void density_reset_opacity_kernel(uint32_t N, float limit, float* __restrict__ logits,
                                                                         float* __restrict__ exp_avg, float* __restrict__ exp_avg_sq,
                                                                         float* __restrict__ out_opacities)
{
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < N; i += gridDim.x * kThreads) {
        const float x = fminf(logits[i], limit);
        logits[i] = x;
        exp_avg[i] = 0.0f;
        exp_avg_sq[i] = 0.0f;
        out_opacities[i] = act_opacity(x);
    }
}

dim3 elementwise_grid(uint32_t n)
{
    const uint32_t blocks = (n + kThreads - 1) / kThreads;
    return dim3(blocks < kMaxGrid ? blocks : kMaxGrid);
}

bool bad_threshold(float x) { return !(x >= 0.0f); }         // negative or NaN

}  // namespace

}  // namespace fs

using namespace fs;

FS_API int fs_density_api_version(void) { return FS_DENSITY_API_VERSION; }

FS_API int fs_density_accumulate(int32_t N, const float* g_means2D, const int32_t* radii, float* grad_accum, float* denom,
                                 float* max_radii, void* stream_)
{
    if (N < 0) return FS_ERR_INVALID_ARG;
    if (N == 0) return FS_OK;
    if (!g_means2D || !radii || !grad_accum || !denom || !max_radii) return FS_ERR_INVALID_ARG;
    hipLaunchKernelGGL(density_accumulate_kernel, elementwise_grid((uint32_t)N), dim3(kThreads), 0, (hipStream_t)stream_,
                       (uint32_t)N, g_means2D, radii, grad_accum, denom, max_radii);
    FS_CHECK_LAUNCH("density_accumulate");
    return FS_OK;
}

FS_API size_t fs_density_plan_scratch_bytes(int32_t N)
{
    if (N <= 0) return 0;
    const size_t nb = ((size_t)N + kScanBlock - 1) / kScanBlock;
    return align_up(4 * nb * sizeof(uint32_t), 256);
}

FS_API int fs_density_plan(int32_t N, const float* grad_accum, const float* denom, const float* max_radii, const float* scales,
                           const float* opacities, float grad_threshold, float dense_scale, float min_opacity,
                           float max_screen_size, float prune_scale, float child_prune_scale, uint8_t* kind, uint32_t* offset,
                           uint32_t* src, int32_t* totals, void* scratch, void* stream_)
{
    if (N < 0 || N >= (1 << 30)) return FS_ERR_INVALID_ARG;              // 2 i + 1 must stay below kSplitTag
    if (bad_threshold(grad_threshold) || bad_threshold(dense_scale) || bad_threshold(min_opacity) ||
        bad_threshold(max_screen_size) || bad_threshold(prune_scale) || bad_threshold(child_prune_scale))
        return FS_ERR_INVALID_ARG;
    if (N == 0) return FS_OK;
    if (!grad_accum || !denom || !max_radii || !scales || !opacities || !kind || !offset || !src || !totals || !scratch)
        return FS_ERR_INVALID_ARG;
    PlanArgs a;
    a.grad_accum = grad_accum; a.denom = denom; a.max_radii = max_radii; a.scales = scales; a.opacities = opacities;
    a.grad_threshold = grad_threshold; a.dense_scale = dense_scale; a.min_opacity = min_opacity;
    a.max_screen_size = max_screen_size; a.prune_scale = prune_scale; a.child_prune_scale = child_prune_scale;
    a.N = (uint32_t)N;
    a.nb = (a.N + kScanBlock - 1) / kScanBlock;
    uint32_t* block_counts = (uint32_t*)scratch;
    hipStream_t st = (hipStream_t)stream_;
    hipLaunchKernelGGL(density_count_kernel, dim3(a.nb), dim3(kThreads), 0, st, a, kind, block_counts);
    hipLaunchKernelGGL(density_scan_blocks_kernel, dim3(1), dim3(kScanThreads), 0, st, a.nb, block_counts, totals);
    hipLaunchKernelGGL(density_emit_kernel, dim3(a.nb), dim3(kThreads), 0, st, a.N, (const uint8_t*)kind,
                       (const uint32_t*)block_counts, offset, src);
    FS_CHECK_LAUNCH("density_plan");
    return FS_OK;
}

FS_API int fs_density_apply(int32_t N, int32_t M, int32_t N_out, const uint32_t* src, const float* const* p_src, const float* const* exp_avg_src, const float* const* exp_avg_sq_src,
                            float* const* p_dst, float* const* exp_avg_dst, float* const* exp_avg_sq_dst, float* out_scales,
                            float* out_opacities, uint32_t seed, void* stream_)
{
    if (N < 0 || N_out < 0 || (M != 1 && M != 4 && M != 9 && M != 16)) return FS_ERR_INVALID_ARG;
    if (3ll * M * N > 0x7FFFFFFFll || 3ll * M * N_out > 0x7FFFFFFFll) return FS_ERR_INVALID_ARG;
    if (N == 0 || N_out == 0) return FS_OK;
    if ((long long)N_out > 2ll * N) return FS_ERR_INVALID_ARG;
    if (!src || !p_src || !exp_avg_src || !exp_avg_sq_src || !p_dst || !exp_avg_dst || !exp_avg_sq_dst || !out_scales ||
        !out_opacities)
        return FS_ERR_INVALID_ARG;
    for (int k = 0; k < FS_OPTIM_ARRAYS; ++k)
        if (!p_src[k] || !exp_avg_src[k] || !exp_avg_sq_src[k] || !p_dst[k] || !exp_avg_dst[k] || !exp_avg_sq_dst[k])
            return FS_ERR_INVALID_ARG;

    const uint32_t widths[FS_OPTIM_ARRAYS] = {3u, 3u, 4u, 1u, 3u * (uint32_t)M};
    ApplyArgs a;
    uint32_t chunks = 0;
    for (int k = 0; k < FS_OPTIM_ARRAYS; ++k) {
        ApplySeg& s = a.seg[k];
        s.ps = p_src[k]; s.ms = exp_avg_src[k]; s.vs = exp_avg_sq_src[k];
        s.pd = p_dst[k]; s.md = exp_avg_dst[k]; s.vd = exp_avg_sq_dst[k];
        s.act = k == FS_OPTIM_SCALES ? out_scales : k == FS_OPTIM_OPACITIES ? out_opacities : nullptr;
        s.len = widths[k] * (uint32_t)N_out;
        s.first_chunk = chunks;
        chunks += (s.len + kChunk - 1) / kChunk;
        s.end_chunk = chunks;
        s.vec_dst = aligned16(s.pd) && aligned16(s.md) && aligned16(s.vd) && aligned16(s.act);
        s.vec_src = aligned16(s.ps) && aligned16(s.ms) && aligned16(s.vs);
    }
    a.src = src;
    a.N = (uint32_t)N; a.seed = seed; a.M = M;
    hipLaunchKernelGGL(density_apply_kernel, dim3(chunks < kMaxGrid ? chunks : kMaxGrid), dim3(kThreads), 0, (hipStream_t)stream_, a);
    FS_CHECK_LAUNCH("density_apply");
    return FS_OK;
}

FS_API int fs_density_reset_opacity(int32_t N, double max_opacity, float* logits, float* exp_avg, float* exp_avg_sq,
                                    float* out_opacities, void* stream_)
{
    if (N < 0 || !(max_opacity > 0.0 && max_opacity < 1.0)) return FS_ERR_INVALID_ARG;
    if (N == 0) return FS_OK;
    if (!logits || !exp_avg || !exp_avg_sq || !out_opacities) return FS_ERR_INVALID_ARG;
    const float limit = (float)log(max_opacity / (1.0 - max_opacity));
    hipLaunchKernelGGL(density_reset_opacity_kernel, elementwise_grid((uint32_t)N), dim3(kThreads), 0, (hipStream_t)stream_,
                       (uint32_t)N, limit, logits, exp_avg, exp_avg_sq, out_opacities);
    FS_CHECK_LAUNCH("density_reset_opacity");
    return FS_OK;
}
