// metrics.hip -- evaluation metrics of FreeSplat's test / validation steps, on the device.
//
// fs_image_metrics: SSIM (skimage.metrics.structural_similarity with win_size=11, gaussian_weights=True,
// channel_axis=0, data_range=1, as src/evaluation/metrics.py:37-52 calls it) and the MSE of compute_psnr
// (metrics.py:11-19) of a batch of views in one launch pair.  The reference copies every view to the host and filters it
// there; here a workgroup owns a strip of kTileW x kTileH output pixels of one (view, channel) plane and runs the two 11-tap
// passes described in ssim_pass.h (whose pieces ssim_loss.hip uses too).  skimage crops 5 pixels, so every kept output has its
// whole window inside the image and no padding is ever read.  Each pixel's squared error is added once, by the thread of its
// column, while the row passes through registers.
//
// fs_depth_metrics: the masked per-view sums behind depth_render_metrics (src/model/model_wrapper.py:90-110).
//
// Deterministic: per-thread fp32 sums in a fixed order, then block_sum_tree and finalize_rows_kernel of fs_reduce.h.  The
// partition of a view into workgroups depends only on (C, H, W) (resp. H*W), so a view's result is the same bits alone or
// inside a batch, on any stream.  No atomics.
#include "ssim_pass.h"

namespace fs {

namespace {

using namespace ssim;

constexpr int kThreads = kSumThreads;
constexpr int kDepthPix = 16;                 // depth pixels per thread

__device__ __forceinline__ float clip01(float v)   // torch.clip: NaN stays NaN
{
    return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
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

    // inputs of rows y0 - 5 + i (i < 10 + kRows) of this column, minus the tile's pivot.  Outside the image 0 (never part of a
    // kept window).  The squared error of a tile's own pixel is added as it loads.
    const float ox = pivot_of(gx_[(size_t)y0 * W + x0]), oy = pivot_of(gy_[(size_t)y0 * W + x0]);
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
        // vertical pass
#pragma unroll
        for (int o = 0; o < kRows; ++o) {
            float m[5];
            column_moments(xr + o, yr + o, w, m);
#pragma unroll
            for (int k = 0; k < 5; ++k) s_m[o][k][t] = m[k];
        }
        __syncthreads();
        // horizontal pass + S
        for (int it = t; it < kRows * kGroups; it += kThreads) {
            const int o = it / kGroups, c0 = 4 * (it - o * kGroups);
            const int yy = y0 + r0 + o;
            float u[5][4];
#pragma unroll
            for (int m = 0; m < 5; ++m) row_taps4(&s_m[o][m][c0], w, u[m]);
            const bool row_in = yy >= kRad && yy < H - kRad;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int xx = x0 + c0 + q;
                const float S = ssim_terms(u[0][q], u[1][q], u[2][q], u[3][q], u[4][q], ox, oy, kF).S;
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
    block_sum_tree<2>(v, reinterpret_cast<double*>(&s_m[0][0][0]));   // (the moments are dead after the last barrier)
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
    block_sum_tree<6>(v, s_red);
    if (t == 0)
#pragma unroll
        for (int f = 0; f < 6; ++f) rows[(size_t)blockIdx.x * 6 + f] = v[f];
}

bool image_args_ok(int32_t B, int32_t C, int32_t H, int32_t W)
{
    if (B <= 0 || C <= 0 || H < kTaps || W < kTaps) return false;
    int tx, tiles;
    plane_tiles(H, W, tx, tiles);
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
    plane_tiles(H, W, tx, tiles);
    return align_up((size_t)B * C * tiles * sizeof(double2), 256);
}

FS_API int fs_image_metrics(int32_t B, int32_t C, int32_t H, int32_t W, const float* gt, const float* pred, double* ssim,
                            double* mse, float* ssim_map, void* scratch, void* stream_)
{
    if (!image_args_ok(B, C, H, W) || !gt || !pred || !ssim || !mse || !scratch) return FS_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream_;
    int tiles_x, tiles;
    plane_tiles(H, W, tiles_x, tiles);
    double2* rows = static_cast<double2*>(scratch);
    hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)(B * C * tiles)), dim3(kThreads), 0, st, H, W, tiles_x, tiles, gt, pred,
                       Weights::make(), ssim_map, rows);
    const RowOuts<2> outs = {{ssim, mse}, {1.0 / ((double)C * (H - 2 * kRad) * (W - 2 * kRad)), 1.0 / ((double)C * H * W)}, 1};
    hipLaunchKernelGGL((finalize_rows_kernel<2, BlockSum::kTree, true>), dim3((unsigned)B), dim3(kThreads), 0, st, C * tiles, 1,
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
    RowOuts<6> outs = {};
    for (int f = 0; f < 6; ++f) outs.out[f] = out + (size_t)f * B;
    outs.stride = 1;
    hipLaunchKernelGGL((finalize_rows_kernel<6, BlockSum::kTree, false>), dim3((unsigned)B), dim3(kThreads), 0, st, chunks, 1,
                       (const double*)rows, outs);
    FS_CHECK_LAUNCH("depth_metrics");
    return FS_OK;
}
