// lpips.hip -- the LPIPS distance head (src/loss/loss_lpips.py:27-55, src/evaluation/metrics.py:22-34) and its input side.
//
// The VGG-16 convolutions of LPIPS stay on torch / MIOpen; what runs here is everything around them:
//   fs_lpips_prepare_forward / _backward: optional 2x - 1, the scaling layer (x - shift_c) / scale_c, and prediction and
//     target packed as one [2B, C, H, W] batch so the convolution stack runs once;
//   fs_lpips_layer_forward: per tap layer, dist[b] += mean_{h,w} sum_c w_c (f0_c / (|f0| + eps) - f1_c / (|f1| + eps))^2,
//     |.| the L2 norm over channels at that pixel, eps = 1e-10;
//   fs_lpips_layer_backward: d dist / d f0 (and d f1) from one read of the maps and four saved floats per pixel.
//
// Geometry (forward and backward): a workgroup owns kPix = 64 consecutive pixels of one image's flattened H x W plane --
// lanes run along W, the stride-1 axis of NCHW, so every channel step of a wavefront is one 256-byte access -- and
// G = ceil(C / kSlots) wavefronts (<= 16) share the channels: wavefront g takes c = g, g + G, g + 2G, ...
// A pixel's channel vector is needed twice, for the norms and then for the differences (the differences are formed
// directly: the expanded form a^2 S00 - 2ab S01 + b^2 S11 reads once but cancels to nothing when prediction ~ target).
// The forward loads its <= kSlots channels of both maps into registers once and makes both visits there (a second global
// read of the tile, served by L2, measured 25 - 48 % slower per forward: profiles/lpips_head_ab.txt); the wavefronts
// combine their partial sums through LDS in the fixed order g = 0 .. G - 1.
//
// Deterministic: a pixel's sums are added in a fixed order (per wavefront over its channels, then over wavefronts); the 64
// pixels of a workgroup in a fixed LDS tree; one partial per workgroup goes to `scratch`; fs_lpips_layer_forward's second
// kernel (one workgroup per image) adds an image's partials in fp64 in a fixed order and adds the mean to dist[b].  The
// partition depends only on (C, H, W): an image's value is the same bits alone or in a batch, on any stream.  No atomics.
//
// Zero-norm pixels: where all C channels of a map are 0, torch's autograd gives NaN (sqrt's backward at 0).  Here
// d|f| / df = 0 there: the gradient is finite and equals 2 w_c d_c / (|f| + eps) with |f| = 0.
#include "fs_common.h"

#include <math.h>

namespace fs {

namespace {

constexpr int kPix = 64;        // pixels per workgroup = one wavefront along W
constexpr int kSlots = 32;      // channels a thread keeps in registers (x 2 maps)
constexpr int kMaxG = 16;       // wavefronts per workgroup
constexpr int kMaxC = kSlots * kMaxG;
constexpr int kFinThreads = 256;
constexpr int kPrepThreads = 256;
constexpr float kEps = 1e-10f;

__host__ __device__ inline int groups_for(int C) { return (C + kSlots - 1) / kSlots; }

// saved: four planes of [B, HW] floats: |f0|, |f1|, T0 = sum_c q_c u_c, T1 = sum_c q_c v_c
// (u = f0 / (|f0| + eps), v = f1 / (|f1| + eps), q_c = 2 w_c (u_c - v_c))
__global__ __launch_bounds__(kPix* kMaxG) void lpips_layer_fwd_kernel(int C, int HW, int tiles, const float* __restrict__ f0,
                                                                       const float* __restrict__ f1,
                                                                       const float* __restrict__ w, float* __restrict__ saved,
                                                                       size_t plane, float* __restrict__ partials)
{
    __shared__ float s_red[4][kMaxG][kPix];
    // g is uniform over a wavefront (blockDim.x = 64): as a scalar it keeps the channel addresses out of the vector registers
    const int lane = threadIdx.x, g = __builtin_amdgcn_readfirstlane(threadIdx.y), G = blockDim.y;
    const int b = blockIdx.y, tile = blockIdx.x;
    const int p = tile * kPix + lane;
    const bool in = p < HW;
    const unsigned po = in ? p : 0;
    const float* __restrict__ q0 = f0 + (size_t)b * C * HW;
    const float* __restrict__ q1 = f1 + (size_t)b * C * HW;
    float x[kSlots], y[kSlots];
    // visit 1: the loads (all in flight at once) and the squared norms
#pragma unroll
    for (int i = 0; i < kSlots; ++i) {
        const int c = g + i * G;
        const bool ok = in && c < C;
        const size_t o = (size_t)(c < C ? c : 0) * HW;
        x[i] = ok ? (q0 + o)[po] : 0.0f;
        y[i] = ok ? (q1 + o)[po] : 0.0f;
    }
    float sx = 0.0f, sy = 0.0f;
#pragma unroll
    for (int i = 0; i < kSlots; ++i) {
        sx = fmaf(x[i], x[i], sx);
        sy = fmaf(y[i], y[i], sy);
    }
    s_red[0][g][lane] = sx;
    s_red[1][g][lane] = sy;
    __syncthreads();
    sx = 0.0f;
    sy = 0.0f;
    for (int k = 0; k < G; ++k) {
        sx += s_red[0][k][lane];
        sy += s_red[1][k][lane];
    }
    const float n0 = sqrtf(sx), n1 = sqrtf(sy);
    const float a = 1.0f / (n0 + kEps), bb = 1.0f / (n1 + kEps);
    // visit 2: the differences, formed directly (identical maps give exactly 0)
    float s = 0.0f, t0 = 0.0f, t1 = 0.0f;
#pragma unroll
    for (int i = 0; i < kSlots; ++i) {
        const int c = g + i * G;
        const float wc = c < C ? w[c] : 0.0f;
        const float u = x[i] * a, v = y[i] * bb;
        const float d = u - v;
        const float wd = wc * d;
        s = fmaf(wd, d, s);
        t0 = fmaf(wd, u, t0);
        t1 = fmaf(wd, v, t1);
    }
    s_red[2][g][lane] = s;
    s_red[3][g][lane] = t0;
    __syncthreads();                 // (also: every wavefront has read planes 0 and 1)
    s_red[0][g][lane] = t1;
    __syncthreads();
    if (g == 0) {
        s = 0.0f;
        t0 = 0.0f;
        t1 = 0.0f;
        for (int k = 0; k < G; ++k) {
            s += s_red[2][k][lane];
            t0 += s_red[3][k][lane];
            t1 += s_red[0][k][lane];
        }
        if (in) {
            const size_t o = (size_t)b * HW + p;
            saved[o] = n0;
            saved[plane + o] = n1;
            saved[2 * plane + o] = 2.0f * t0;
            saved[3 * plane + o] = 2.0f * t1;
        }
        // the 64 pixels in a fixed tree on plane 1 (dead since the second barrier)
        s_red[1][0][lane] = in ? s : 0.0f;
    }
    __syncthreads();
    for (int h = kPix / 2; h > 0; h >>= 1) {
        if (g == 0 && lane < h) s_red[1][0][lane] += s_red[1][0][lane + h];
        __syncthreads();
    }
    if (g == 0 && lane == 0) partials[(size_t)b * tiles + tile] = s_red[1][0][0];
}

// one workgroup per image: dist[b] += (sum of the image's partials, fp64, fixed order) / HW
__global__ __launch_bounds__(kFinThreads) void lpips_finish_kernel(int tiles, double inv_hw, const float* __restrict__ partials,
                                                                   float* __restrict__ dist)
{
    __shared__ double s_red[kFinThreads];
    const int t = threadIdx.x, b = blockIdx.x;
    const float* r = partials + (size_t)b * tiles;
    double v = 0.0;
    for (int k = t; k < tiles; k += kFinThreads) v += (double)r[k];
    s_red[t] = v;
    __syncthreads();
    for (int s = kFinThreads / 2; s > 0; s >>= 1) {
        if (t < s) s_red[t] += s_red[t + s];
        __syncthreads();
    }
    if (t == 0) dist[b] += (float)(s_red[0] * inv_hw);
}

// g_f0_c = gs (a q_c - u_c T0 / |f0|),  g_f1_c = gs (-b q_c + v_c T1 / |f1|),  gs = g_dist[b] / HW; the second term is
// dropped where the norm is 0 (file header)
__global__ __launch_bounds__(kPix* kMaxG) void lpips_layer_bwd_kernel(int C, int HW, float inv_hw,
                                                                       const float* __restrict__ g_dist,
                                                                       const float* __restrict__ f0, const float* __restrict__ f1,
                                                                       const float* __restrict__ w,
                                                                       const float* __restrict__ saved, size_t plane,
                                                                       float* __restrict__ g_f0, float* __restrict__ g_f1)
{
    const int lane = threadIdx.x, g = threadIdx.y, G = blockDim.y;
    const int b = blockIdx.y;
    const int p = blockIdx.x * kPix + lane;
    if (p >= HW) return;
    const size_t o = (size_t)b * HW + p;
    const float n0 = saved[o], n1 = saved[plane + o], t0 = saved[2 * plane + o], t1 = saved[3 * plane + o];
    const float gs = g_dist[b] * inv_hw;
    const float a = 1.0f / (n0 + kEps), bb = 1.0f / (n1 + kEps);
    const float r0 = n0 > 0.0f ? t0 / n0 : 0.0f, r1 = n1 > 0.0f ? t1 / n1 : 0.0f;
    const size_t base = (size_t)b * C * HW + p;
#pragma unroll 8
    for (int c = g; c < C; c += G) {
        const size_t i = base + (size_t)c * HW;
        const float u = f0[i] * a, v = f1[i] * bb;
        const float q = 2.0f * (w[c] * (u - v));
        if (g_f0) g_f0[i] = gs * (a * q - u * r0);
        if (g_f1) g_f1[i] = gs * (v * r1 - bb * q);
    }
}

// out [2B, C, HW]: image b < B from in0, image B + b from in1
__global__ __launch_bounds__(kPrepThreads) void lpips_prepare_fwd_kernel(long long n_half, int C, int HW, int normalize,
                                                                        const float* __restrict__ in0,
                                                                        const float* __restrict__ in1,
                                                                        const float* __restrict__ shift,
                                                                        const float* __restrict__ scale, float* __restrict__ out)
{
    const long long i = (long long)blockIdx.x * kPrepThreads + threadIdx.x;
    if (i >= 2 * n_half) return;
    const bool second = i >= n_half;
    const long long j = second ? i - n_half : i;
    const int c = (int)((j / HW) % C);
    float v = second ? in1[j] : in0[j];
    if (normalize) v = 2.0f * v - 1.0f;
    out[i] = (v - shift[c]) / scale[c];
}

__global__ __launch_bounds__(kPrepThreads) void lpips_prepare_bwd_kernel(long long n_half, int C, int HW, int normalize,
                                                                        const float* __restrict__ g_out,
                                                                        const float* __restrict__ scale, float* __restrict__ g_in0,
                                                                        float* __restrict__ g_in1)
{
    const long long i = (long long)blockIdx.x * kPrepThreads + threadIdx.x;
    if (i >= 2 * n_half) return;
    const bool second = i >= n_half;
    float* dst = second ? g_in1 : g_in0;
    if (!dst) return;
    const long long j = second ? i - n_half : i;
    const int c = (int)((j / HW) % C);
    const float v = g_out[i] / scale[c];
    dst[j] = normalize ? 2.0f * v : v;
}

bool layer_args_ok(int32_t B, int32_t C, int32_t H, int32_t W)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || C > kMaxC || B > 65535) return false;
    const long long hw = (long long)H * W;
    return hw <= 0x7fffffffLL - kPix && (long long)B * C * hw <= (1LL << 40);
}

int layer_tiles(int32_t H, int32_t W) { return (int)(((long long)H * W + kPix - 1) / kPix); }

bool prepare_args_ok(int32_t B, int32_t C, int32_t H, int32_t W)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return false;
    const long long hw = (long long)H * W;
    return hw <= 0x7fffffffLL && 2LL * B * C * hw <= (long long)kPrepThreads * 0x7fffffffLL;
}

}  // namespace

}  // namespace fs

using namespace fs;

FS_API size_t fs_lpips_scratch_bytes(int32_t B, int32_t C, int32_t H, int32_t W)
{
    if (!layer_args_ok(B, C, H, W)) return 0;
    return align_up((size_t)B * layer_tiles(H, W) * sizeof(float), 256);
}

FS_API size_t fs_lpips_saved_bytes(int32_t B, int32_t C, int32_t H, int32_t W)
{
    if (!layer_args_ok(B, C, H, W)) return 0;
    return (size_t)4 * B * H * W * sizeof(float);
}

FS_API int fs_lpips_layer_forward(const float* f0, const float* f1, const float* w, int32_t B, int32_t C, int32_t H, int32_t W,
                                  float* dist, float* saved, void* scratch, void* stream_)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || !f0 || !f1 || !w || !dist || !saved || !scratch) return FS_ERR_INVALID_ARG;
    if (C > kMaxC) return FS_ERR_UNSUPPORTED;
    if (!layer_args_ok(B, C, H, W)) return FS_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream_;
    const int HW = H * W, tiles = layer_tiles(H, W);
    float* partials = static_cast<float*>(scratch);
    hipLaunchKernelGGL(lpips_layer_fwd_kernel, dim3((unsigned)tiles, (unsigned)B), dim3(kPix, groups_for(C)), 0, st, C, HW, tiles,
                       f0, f1, w, saved, (size_t)B * HW, partials);
    hipLaunchKernelGGL(lpips_finish_kernel, dim3((unsigned)B), dim3(kFinThreads), 0, st, tiles, 1.0 / (double)HW, partials, dist);
    FS_CHECK_LAUNCH("lpips_layer_forward");
    return FS_OK;
}

FS_API int fs_lpips_layer_backward(const float* g_dist, const float* f0, const float* f1, const float* w, const float* saved,
                                   int32_t B, int32_t C, int32_t H, int32_t W, float* g_f0, float* g_f1, void* stream_)
{
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || !g_dist || !f0 || !f1 || !w || !saved || (!g_f0 && !g_f1)) return FS_ERR_INVALID_ARG;
    if (C > kMaxC) return FS_ERR_UNSUPPORTED;
    if (!layer_args_ok(B, C, H, W)) return FS_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream_;
    const int HW = H * W;
    // 4 wavefronts share a pixel tile's channels (no staging here: each channel is read once and its gradient written)
    const int G = min(groups_for(C), 4);
    hipLaunchKernelGGL(lpips_layer_bwd_kernel, dim3((unsigned)layer_tiles(H, W), (unsigned)B), dim3(kPix, G), 0, st, C, HW,
                       (float)(1.0 / (double)HW), g_dist, f0, f1, w, saved, (size_t)B * HW, g_f0, g_f1);
    FS_CHECK_LAUNCH("lpips_layer_backward");
    return FS_OK;
}

FS_API int fs_lpips_prepare_forward(const float* in0, const float* in1, const float* shift, const float* scale, int32_t B,
                                    int32_t C, int32_t H, int32_t W, int32_t normalize, float* out, void* stream_)
{
    if (!prepare_args_ok(B, C, H, W) || !in0 || !in1 || !shift || !scale || !out) return FS_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream_;
    const long long n_half = (long long)B * C * H * W;
    const unsigned blocks = (unsigned)((2 * n_half + kPrepThreads - 1) / kPrepThreads);
    hipLaunchKernelGGL(lpips_prepare_fwd_kernel, dim3(blocks), dim3(kPrepThreads), 0, st, n_half, C, H * W, normalize, in0, in1,
                       shift, scale, out);
    FS_CHECK_LAUNCH("lpips_prepare_forward");
    return FS_OK;
}

FS_API int fs_lpips_prepare_backward(const float* g_out, const float* scale, int32_t B, int32_t C, int32_t H, int32_t W,
                                     int32_t normalize, float* g_in0, float* g_in1, void* stream_)
{
    if (!prepare_args_ok(B, C, H, W) || !g_out || !scale || (!g_in0 && !g_in1)) return FS_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream_;
    const long long n_half = (long long)B * C * H * W;
    const unsigned blocks = (unsigned)((2 * n_half + kPrepThreads - 1) / kPrepThreads);
    hipLaunchKernelGGL(lpips_prepare_bwd_kernel, dim3(blocks), dim3(kPrepThreads), 0, st, n_half, C, H * W, normalize, g_out,
                       scale, g_in0, g_in1);
    FS_CHECK_LAUNCH("lpips_prepare_backward");
    return FS_OK;
}
