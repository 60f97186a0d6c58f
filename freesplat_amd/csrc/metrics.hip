// metrics.hip -- evaluation metrics of FreeSplat's test / validation steps, on the device.
//
// fs_image_metrics: SSIM (skimage.metrics.structural_similarity with win_size=11, gaussian_weights=True,
// channel_axis=0, data_range=1, as src/evaluation/metrics.py:37-52 calls it) and the MSE of compute_psnr
// (metrics.py:11-19) of a batch of views in one launch pair.  The reference copies every view to the host and filters it
// there; here a workgroup owns a strip of kTileW x kTileH output pixels of one (view, channel) plane:
//   vertical 11-tap pass: one thread per patch column (kTileW + 10 = 256), sliding down the rows with the inputs of the
//     last 10 + kRows rows in registers; the five moments x, y, x^2, y^2, xy of kRows rows go to LDS;
//   horizontal 11-tap pass: a thread takes 4 consecutive output pixels of a row (16-byte LDS reads), forms S and adds
//     it to its partial when the window lies inside the image (skimage crops 5 pixels, so every kept output has its whole
//     window inside the image and no padding is ever read).
// Each pixel's squared error is added once, by the thread of its column, while the row passes through registers.
//
// fs_depth_metrics: the masked per-view sums behind depth_render_metrics (src/model/model_wrapper.py:90-110).
//
// Deterministic: a thread adds its terms in fp32 in a fixed order, a workgroup adds its threads' partials in fp64 in a
// fixed tree and stores one partial row; a finalize kernel (one workgroup per view) adds a view's rows in a fixed order.
// The partition of a view into workgroups depends only on (C, H, W) (resp. H*W), so a view's result is the same bits
// alone or inside a batch, on any stream.  No atomics.
#include "fs_common.h"

#include <math.h>

namespace fs {

namespace {

constexpr int kThreads = 256;
constexpr int kRad = 5;                       // sigma 1.5, truncate 3.5: int(3.5 * 1.5 + 0.5)
constexpr int kTaps = 2 * kRad + 1;
constexpr int kTileW = kThreads - 2 * kRad;   // 246 output columns: patch column = thread
constexpr int kTileH = 64;                    // output rows per workgroup
constexpr int kRows = 8;                      // output rows per LDS round
constexpr int kGroups = (kTileW + 3) / 4;     // 62 groups of 4 output columns in the horizontal pass
constexpr int kLdsRow = 260;                  // >= 4 * (kGroups - 1) + 16: the last group's 16-byte reads stay in the row
constexpr int kDepthPix = 16;                 // depth pixels per thread

struct Weights {
    float w[kTaps];
};

__device__ __forceinline__ float clip01(float v)   // torch.clip: NaN stays NaN
{
    return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
}

// fixed-order fp64 tree over the 256 threads of a workgroup; returns the total in thread 0
template <int F>
__device__ __forceinline__ void block_sum(double (&v)[F], double* s_red /* [F][kThreads] */)
{
    const int t = threadIdx.x;
#pragma unroll
    for (int f = 0; f < F; ++f) s_red[f * kThreads + t] = v[f];
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if (t < s)
#pragma unroll
            for (int f = 0; f < F; ++f) s_red[f * kThreads + t] += s_red[f * kThreads + t + s];
        __syncthreads();
    }
#pragma unroll
    for (int f = 0; f < F; ++f) v[f] = s_red[f * kThreads];
}

// One (view, channel) plane tile.  blockIdx.x = plane * tiles + tile; rows[blockIdx.x] = (sum of S, sum of squared error).
__global__ __launch_bounds__(kThreads) void ssim_tile_kernel(int H, int W, int tiles_x, int tiles, const float* __restrict__ gt,
                                                             const float* __restrict__ pred, Weights wt,
                                                             float* __restrict__ ssim_map, double2* __restrict__ rows)
{
    __shared__ __attribute__((aligned(16))) float s_m[kRows][5][kLdsRow];
    const int t = threadIdx.x;
    const long long plane = blockIdx.x / tiles;
    const int tile = blockIdx.x - (int)(plane * tiles);
    const int x0 = (tile % tiles_x) * kTileW, y0 = (tile / tiles_x) * kTileH;
    const size_t base = (size_t)plane * H * W;
    const float* __restrict__ gx_ = gt + base;
    const float* __restrict__ gy_ = pred + base;
    const int col = x0 - kRad + t;                           // this thread's image column in the vertical pass
    const bool col_in = col >= 0 && col < W;
    const bool col_own = t >= kRad && t < kRad + kTileW && col < W;   // the tile's own column: its squared error is ours
    float w[kTaps];
#pragma unroll
    for (int k = 0; k < kTaps; ++k) w[k] = wt.w[k];
    constexpr float kF = 121.0f / 120.0f;                    // use_sample_covariance: NP / (NP - 1), NP = 11^2
    constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;

    // inputs of rows y0 - 5 + i (i < 10 + kRows) of this column, minus an offset: the moments are taken about the value of
    // the tile's first pixel in each image (0.5 where it is not finite or lies outside [-1, 2]), which keeps u_xx - u_x^2 from
    // cancelling away the variance of smooth images (4 - 8x smaller per-pixel error than raw values) and makes every
    // variance of a constant image exactly 0.  Outside the image 0 (never part of a kept window).  The squared error of a
    // tile's own pixel is added as it loads.
    auto offset = [](float v) { return v >= -1.0f && v <= 2.0f ? v : 0.5f; };
    const float ox = offset(gx_[(size_t)y0 * W + x0]), oy = offset(gy_[(size_t)y0 * W + x0]);
    const int y_end = min(y0 + kTileH, H);
    float xr[kRows + 2 * kRad], yr[kRows + 2 * kRad];
    float s_sum = 0.0f, e_sum = 0.0f;
    auto load = [&](int r, float& a, float& b) __attribute__((always_inline)) {
        const bool in = col_in && r >= 0 && r < H;
        const size_t o = in ? (size_t)r * W + col : 0;
        const float xa = in ? gx_[o] : 0.0f, ya = in ? gy_[o] : 0.0f;
        const float d = clip01(xa) - clip01(ya);             // compute_psnr's clipped error
        if (col_own && r >= y0 && r < y_end) e_sum += d * d;
        a = xa - ox;
        b = ya - oy;
    };
#pragma unroll
    for (int i = 0; i < 2 * kRad; ++i) load(y0 - kRad + i, xr[i], yr[i]);

    for (int r0 = 0; r0 < kTileH; r0 += kRows) {
        if (y0 + r0 >= H) break;                             // (workgroup-uniform; every row < H is loaded by now)
#pragma unroll
        for (int i = 0; i < kRows; ++i) load(y0 + r0 + kRad + i, xr[2 * kRad + i], yr[2 * kRad + i]);
        // vertical pass: the x- and y-terms take identical operation sequences (identical images give S = 1 exactly)
#pragma unroll
        for (int o = 0; o < kRows; ++o) {
            float ux = 0.0f, uy = 0.0f, uxx = 0.0f, uyy = 0.0f, uxy = 0.0f;
#pragma unroll
            for (int k = 0; k < kTaps; ++k) {
                const float x = xr[o + k], y = yr[o + k];
                const float wx = w[k] * x, wy = w[k] * y;
                ux += wx;
                uy += wy;
                uxx = fmaf(wx, x, uxx);
                uyy = fmaf(wy, y, uyy);
                uxy = fmaf(wx, y, uxy);
            }
            s_m[o][0][t] = ux; s_m[o][1][t] = uy; s_m[o][2][t] = uxx; s_m[o][3][t] = uyy; s_m[o][4][t] = uxy;
        }
        __syncthreads();
        // horizontal pass + S
        for (int it = t; it < kRows * kGroups; it += kThreads) {
            const int o = it / kGroups, c0 = 4 * (it - o * kGroups);
            const int yy = y0 + r0 + o;
            float u[5][4];
#pragma unroll
            for (int m = 0; m < 5; ++m) {
                float v[16];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float4 f = *reinterpret_cast<const float4*>(&s_m[o][m][c0 + 4 * q]);
                    v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    float a = 0.0f;
#pragma unroll
                    for (int k = 0; k < kTaps; ++k) a = fmaf(w[k], v[q + k], a);
                    u[m][q] = a;
                }
            }
            const bool row_in = yy >= kRad && yy < H - kRad;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int xx = x0 + c0 + q;
                const float cx = u[0][q], cy = u[1][q];       // (means of the centred values)
                const float vx = kF * (u[2][q] - cx * cx);
                const float vy = kF * (u[3][q] - cy * cy);
                const float vxy = kF * (u[4][q] - cx * cy);
                const float ux = cx + ox, uy = cy + oy;
                const float a1 = 2.0f * (ux * uy) + kC1, a2 = 2.0f * vxy + kC2;
                const float b1 = (ux * ux + uy * uy) + kC1, b2 = (vx + vy) + kC2;
                const float S = (a1 * a2) / (b1 * b2);
                if (row_in && c0 + q < kTileW && xx >= kRad && xx < W - kRad) {
                    s_sum += S;
                    if (ssim_map)
                        ssim_map[(size_t)plane * (H - 2 * kRad) * (W - 2 * kRad) + (size_t)(yy - kRad) * (W - 2 * kRad) +
                                 (xx - kRad)] = S;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2 * kRad; ++i) { xr[i] = xr[kRows + i]; yr[i] = yr[kRows + i]; }
    }
    double v[2] = {(double)s_sum, (double)e_sum};
    block_sum<2>(v, reinterpret_cast<double*>(&s_m[0][0][0]));   // (the moments are dead after the last barrier)
    if (t == 0) rows[blockIdx.x] = make_double2(v[0], v[1]);
}

// per view: n_valid, n_nonnan, sum |gt - pred|, sum |gt - pred| / gt, n(delta < 1.25), n(delta < 1.1)
__global__ __launch_bounds__(kThreads) void depth_metrics_kernel(long long HW, int chunks, const float* __restrict__ gt,
                                                                 const float* __restrict__ pred, float thresh,
                                                                 double* __restrict__ rows)
{
    __shared__ double s_red[6 * kThreads];
    const int t = threadIdx.x;
    const long long view = blockIdx.x / chunks;
    const int chunk = blockIdx.x - (int)(view * chunks);
    const float* __restrict__ g = gt + view * HW;
    const float* __restrict__ p = pred + view * HW;
    int n_valid = 0, n_nonnan = 0, n25 = 0, n10 = 0;
    float s_abs = 0.0f, s_rel = 0.0f;
#pragma unroll 4
    for (int i = 0; i < kDepthPix; ++i) {
        const long long px = (long long)chunk * (kThreads * kDepthPix) + (long long)i * kThreads + t;
        if (px >= HW) break;
        const float gv = g[px], pv = p[px];
        if (!(gv > thresh)) continue;                        // gt <= 0.5 (or NaN) is masked out
        ++n_valid;
        const float d = fabsf(gv - pv);
        if (!isnan(d)) {                                     // torch.nanmean drops NaN terms
            ++n_nonnan;
            s_abs += d;
            s_rel += d / gv;
        }
        const float r1 = gv / pv, r2 = pv / gv;              // max(r1, r2) < th, a NaN ratio counting as false
        n25 += (r1 < 1.25f && r2 < 1.25f) ? 1 : 0;
        n10 += (r1 < 1.1f && r2 < 1.1f) ? 1 : 0;
    }
    double v[6] = {(double)n_valid, (double)n_nonnan, (double)s_abs, (double)s_rel, (double)n25, (double)n10};
    block_sum<6>(v, s_red);
    if (t == 0)
#pragma unroll
        for (int f = 0; f < 6; ++f) rows[(size_t)blockIdx.x * 6 + f] = v[f];
}

// one workgroup per view: out[f][view] = scale[f] * (sum of the view's K rows of F doubles, in a fixed order)
template <int F>
struct Outs {
    double* out[F];
    double scale[F];
};
template <int F>
__global__ __launch_bounds__(kThreads) void finalize_rows_kernel(int K, const double* __restrict__ rows, Outs<F> outs)
{
    __shared__ double s_red[F * kThreads];
    const int view = blockIdx.x;
    const double* r = rows + (size_t)view * K * F;
    double v[F];
#pragma unroll
    for (int f = 0; f < F; ++f) v[f] = 0.0;
    for (int k = threadIdx.x; k < K; k += kThreads)
#pragma unroll
        for (int f = 0; f < F; ++f) v[f] += r[(size_t)k * F + f];
    block_sum<F>(v, s_red);
    if (threadIdx.x == 0)
#pragma unroll
        for (int f = 0; f < F; ++f) outs.out[f][view] = v[f] * outs.scale[f];
}

void image_tiles(int H, int W, int& tiles_x, int& tiles)
{
    tiles_x = (W + kTileW - 1) / kTileW;
    tiles = tiles_x * ((H + kTileH - 1) / kTileH);
}

bool image_args_ok(int32_t B, int32_t C, int32_t H, int32_t W)
{
    if (B <= 0 || C <= 0 || H < kTaps || W < kTaps) return false;
    int tx, tiles;
    image_tiles(H, W, tx, tiles);
    return (long long)B * C * tiles <= 0x7fffffffLL && (long long)H * W <= 0x7fffffffLL;
}

int depth_chunks(int64_t HW) { return (int)((HW + kThreads * kDepthPix - 1) / (kThreads * kDepthPix)); }

bool depth_args_ok(int32_t B, int64_t HW)
{
    return B > 0 && HW > 0 && (long long)B * depth_chunks(HW) <= 0x7fffffffLL;
}

}  // namespace

}  // namespace fs

using namespace fs;

FS_API size_t fs_image_metrics_scratch_bytes(int32_t B, int32_t C, int32_t H, int32_t W)
{
    if (!image_args_ok(B, C, H, W)) return 0;
    int tx, tiles;
    image_tiles(H, W, tx, tiles);
    return align_up((size_t)B * C * tiles * sizeof(double2), 256);
}

FS_API int fs_image_metrics(int32_t B, int32_t C, int32_t H, int32_t W, const float* gt, const float* pred, double* ssim,
                            double* mse, float* ssim_map, void* scratch, void* stream_)
{
    if (!image_args_ok(B, C, H, W) || !gt || !pred || !ssim || !mse || !scratch) return FS_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream_;
    int tiles_x, tiles;
    image_tiles(H, W, tiles_x, tiles);
    // Gaussian weights as scipy.ndimage builds them: exp(-k^2 / (2 sigma^2)) normalised in double, k = -5..5
    Weights wt;
    double e[kTaps], sum = 0.0;
    for (int k = 0; k < kTaps; ++k) {
        const double d = k - kRad;
        e[k] = exp(-0.5 * d * d / (1.5 * 1.5));
        sum += e[k];
    }
    for (int k = 0; k < kTaps; ++k) wt.w[k] = (float)(e[k] / sum);
    double2* rows = static_cast<double2*>(scratch);
    hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)(B * C * tiles)), dim3(kThreads), 0, st, H, W, tiles_x, tiles, gt, pred,
                       wt, ssim_map, rows);
    Outs<2> outs;
    outs.out[0] = ssim;
    outs.out[1] = mse;
    outs.scale[0] = 1.0 / ((double)C * (H - 2 * kRad) * (W - 2 * kRad));
    outs.scale[1] = 1.0 / ((double)C * H * W);
    hipLaunchKernelGGL(finalize_rows_kernel<2>, dim3((unsigned)B), dim3(kThreads), 0, st, C * tiles,
                       reinterpret_cast<const double*>(rows), outs);
    FS_CHECK_LAUNCH("image_metrics");
    return FS_OK;
}

FS_API size_t fs_depth_metrics_scratch_bytes(int32_t B, int64_t HW)
{
    if (!depth_args_ok(B, HW)) return 0;
    return align_up((size_t)B * depth_chunks(HW) * 6 * sizeof(double), 256);
}

FS_API int fs_depth_metrics(int32_t B, int64_t HW, const float* gt, const float* pred, float threshold, double* out,
                            void* scratch, void* stream_)
{
    if (!depth_args_ok(B, HW) || !gt || !pred || !out || !scratch) return FS_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream_;
    const int chunks = depth_chunks(HW);
    double* rows = static_cast<double*>(scratch);
    hipLaunchKernelGGL(depth_metrics_kernel, dim3((unsigned)(B * chunks)), dim3(kThreads), 0, st, (long long)HW, chunks, gt,
                       pred, threshold, rows);
    Outs<6> outs;
    for (int f = 0; f < 6; ++f) {
        outs.out[f] = out + (size_t)f * B;
        outs.scale[f] = 1.0;
    }
    hipLaunchKernelGGL(finalize_rows_kernel<6>, dim3((unsigned)B), dim3(kThreads), 0, st, chunks, rows, outs);
    FS_CHECK_LAUNCH("depth_metrics");
    return FS_OK;
}
