// ssim_loss.hip -- differentiable SSIM + L1 photometric loss (include/freesplat_amd_loss.h), forward and backward.
//
// The forward is the tiled pass of metrics.hip's ssim_tile_kernel, built from the same pieces (ssim_pass.h), with two
// conventions behind one template parameter (PAD = false: skimage's cropped SSIM; PAD = true: the zero-padded `same` form of
// 3DGS-style training code) and |pred - gt| in place of the squared error; when a backward will follow it stores the three
// partial-derivative maps of every averaged output (12 bytes).  The two kernel bodies stay apart: merged into one inlined
// function template they compile to 14 - 17 more VGPRs each (DESIGN.md "Helper headers").
//
// The backward is a gather: a workgroup owns kTileW x kTileH pixels of g_pred, runs the same two passes over the three
// saved maps (zero outside the averaged outputs) and combines them with pred and gt of the pixel.  Every pixel of g_pred is
// written by exactly one thread; nothing is accumulated in memory.
//
// Deterministic as metrics.hip: per-thread fp32 sums in a fixed order (|pred - gt| in fp64), then block_sum_tree and
// finalize_rows_kernel of fs_reduce.h.  The partition depends only on (C, H, W).  No atomics.
#include "ssim_pass.h"

#include "../../include/freesplat_amd_loss.h"

namespace fs {

namespace {

using namespace ssim;

constexpr int kThreads = kSumThreads;

// One (view, channel) plane tile.  blockIdx.x = plane * tiles + tile; rows[blockIdx.x] = (sum of S, sum of |pred - gt|).
// x = gt, y = pred (the side that gets the gradient).  saved: NULL or [planes][3][Hm][Wm] with (Hm, Wm) the averaged
// outputs, (H - 10, W - 10) or (H, W); SAVE = false leaves the maps' arithmetic out (no backward will follow).
template <bool PAD, bool SAVE>
__global__ __launch_bounds__(kThreads) void ssim_loss_fwd_kernel(int H, int W, int tiles_x, int tiles,
                                                                 const float* __restrict__ pred, const float* __restrict__ gt,
                                                                 Weights wt, float* __restrict__ saved,
                                                                 double2* __restrict__ rows)
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
    const bool col_own = t >= kRad && t < kRad + kTileW && col < W;   // the tile's own column: its |pred - gt| is ours
    const int off = PAD ? 0 : kRad;                          // output (yy, xx) is entry (yy - off, xx - off) of the maps
    const int Hm = H - 2 * off, Wm = W - 2 * off;
    float* __restrict__ sv = SAVE ? saved + (size_t)plane * 3 * Hm * Wm : nullptr;
    float w[kTaps];
#pragma unroll
    for (int k = 0; k < kTaps; ++k) w[k] = wt.w[k];
    constexpr float kF = PAD ? 1.0f : 121.0f / 120.0f;       // population / sample covariance (NP / (NP - 1), NP = 11^2)

    // The per-tile pivot (pivot_of) under padding.  A pixel outside the image is the raw value 0 (the zero padding of PAD; never
    // part of a kept window otherwise), i.e. -pivot here: the weights sum to 1 over the whole window, so the shift stays exact
    // under padding.  A tile whose patch reaches into the padding takes HALF the pivot, midway between the padding and the
    // image, so that neither side's centred magnitude exceeds the raw one (about the pixel value itself the padding of a bright
    // image is as far from the pivot as it can be: 4x the gradient error at 11 x 11 with values up to 1.4).  An image smaller
    // than the window keeps its raw values (pivot 0): there a window is mostly padding and u = pivot + (mean of the centred
    // values) would cancel down to the small in-image weight (1 x 1: 0.07); with an image of at least 11 in both axes a window
    // keeps >= 0.4 of its weight inside.
    const bool raw = PAD && (H < kTaps || W < kTaps);
    const bool edge = PAD && (x0 < kRad || y0 < kRad || x0 + kTileW + kRad > W || y0 + kTileH + kRad > H);
    const float pivot_scale = raw ? 0.0f : (edge ? 0.5f : 1.0f);
    const float ox = pivot_scale * pivot_of(gx_[(size_t)y0 * W + x0]), oy = pivot_scale * pivot_of(gy_[(size_t)y0 * W + x0]);
    const int y_end = min(y0 + kTileH, H);
    float xr[kRows + 2 * kRad], yr[kRows + 2 * kRad];
    float s_sum = 0.0f;
    double l_sum = 0.0;
    auto load = [&](int r, float& a, float& b) __attribute__((always_inline)) {
        const bool in = col_in && r >= 0 && r < H;
        const size_t o = in ? (size_t)r * W + col : 0;
        const float xa = in ? gx_[o] : 0.0f, ya = in ? gy_[o] : 0.0f;
        if (col_own && r >= y0 && r < y_end) l_sum += (double)fabsf(ya - xa);
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
        // horizontal pass + S (+ the three maps)
        for (int it = t; it < kRows * kGroups; it += kThreads) {
            const int o = it / kGroups, c0 = 4 * (it - o * kGroups);
            const int yy = y0 + r0 + o;
            float u[5][4];
#pragma unroll
            for (int m = 0; m < 5; ++m) row_taps4(&s_m[o][m][c0], w, u[m]);
            const bool row_out = PAD ? yy < H : (yy >= kRad && yy < H - kRad);
            // columns of this group that are averaged outputs form one run [lo, hi) of q (the tile, the image and, without
            // padding, the crop each cut an interval)
            const int xx0 = x0 + c0;
            const int lo = PAD ? 0 : max(0, kRad - xx0);
            const int hi = row_out ? min(min(4, kTileW - c0), (PAD ? W : W - kRad) - xx0) : 0;
            float p_yy[4], p_xy[4], p_y[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const Terms T = ssim_terms(u[0][q], u[1][q], u[2][q], u[3][q], u[4][q], ox, oy, kF);
                if (q >= lo && q < hi) s_sum += T.S;
                if constexpr (!SAVE) continue;
                // dS/d(G*y^2), dS/d(G*xy) and dS/d(G*y) with the two products' 0.5 moved into the last one.  Written so that
                // identical images (a1 == b1, a2 == b2, S == 1 bit for bit) give P_xy == -2 P_yy and P_y == 0 exactly: the
                // two ratios that must be 1 there are true divisions, the common factors 1-ulp reciprocals.
                const float inv_b2 = kF * __builtin_amdgcn_rcpf(T.b2);
                p_yy[q] = -(T.S * inv_b2);
                p_xy[q] = 2.0f * ((T.a1 / T.b1) * inv_b2);
                const float dx = T.cx + (ox - kMid), dy = T.cy + (oy - kMid);
                p_y[q] = (2.0f * __builtin_amdgcn_rcpf(T.b1)) * (T.ux * (T.a2 / T.b2) - T.uy * T.S) - ((2.0f * dy) * p_yy[q] + dx * p_xy[q]);
            }
            if (SAVE && hi > lo) {
                const size_t ro = (size_t)(yy - off) * Wm;
                const size_t mp = (size_t)Hm * Wm;
                if (lo == 0) {
                    const int n = xx0 - off + hi;             // store_row4 writes columns [xx0 - off, n)
                    store_row4(sv + ro, xx0 - off, n, p_yy);
                    store_row4(sv + mp + ro, xx0 - off, n, p_xy);
                    store_row4(sv + 2 * mp + ro, xx0 - off, n, p_y);
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (q >= lo && q < hi) {
                            const size_t i = ro + (size_t)(xx0 + q - off);
                            sv[i] = p_yy[q]; sv[mp + i] = p_xy[q]; sv[2 * mp + i] = p_y[q];
                        }
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 2 * kRad; ++i) { xr[i] = xr[kRows + i]; yr[i] = yr[kRows + i]; }
    }
    double v[2] = {(double)s_sum, l_sum};
    block_sum_tree<2>(v, reinterpret_cast<double*>(&s_m[0][0][0]));   // (the moments are dead after the last barrier)
    if (t == 0) rows[blockIdx.x] = make_double2(v[0], v[1]);
}

// One kTileW x kTileH tile of g_pred of one plane.  The maps are read at rows / columns q - 10 + s + k (k < 11) of the
// [Hm, Wm] maps, s = 5 with padding (a `same` pass) and 0 without (the maps zero-extended by 10), zero outside.
// scale_ssim = 1 / (averaged outputs of a view), scale_l1 = 1 / (C H W); the cotangents are read from device memory.
template <bool PAD>
__global__ __launch_bounds__(kThreads) void ssim_loss_bwd_kernel(int C, int H, int W, int tiles_x, int tiles,
                                                                 const float* __restrict__ pred, const float* __restrict__ gt,
                                                                 const float* __restrict__ g_ssim, const float* __restrict__ g_l1,
                                                                 const float* __restrict__ saved, float scale_ssim,
                                                                 float scale_l1, Weights wt, float* __restrict__ g_pred)
{
    __shared__ __attribute__((aligned(16))) float s_m[kRows][3][kLdsRow];
    const int t = threadIdx.x;
    const long long plane = blockIdx.x / tiles;
    const int tile = blockIdx.x - (int)(plane * tiles);
    const int view = (int)(plane / C);
    const int x0 = (tile % tiles_x) * kTileW, y0 = (tile / tiles_x) * kTileH;
    const size_t base = (size_t)plane * H * W;
    const int off = PAD ? 0 : kRad;
    const int Hm = H - 2 * off, Wm = W - 2 * off;
    const int shift = (PAD ? kRad : 0) - 2 * kRad;           // first map row / column of a pixel's window, relative to it
    const bool has_ssim = g_ssim != nullptr;                 // (kernel-uniform)
    const float gs = has_ssim ? g_ssim[view] * scale_ssim : 0.0f;
    const float gl = g_l1 ? g_l1[view] * scale_l1 : 0.0f;
    const size_t mp = (size_t)Hm * Wm;
    const float* __restrict__ sv = has_ssim ? saved + (size_t)plane * 3 * mp : nullptr;
    const int mcol = x0 + shift + t;                         // this thread's map column in the vertical pass
    const bool col_in = mcol >= 0 && mcol < Wm;
    float w[kTaps];
#pragma unroll
    for (int k = 0; k < kTaps; ++k) w[k] = wt.w[k];

    float m0[kRows + 2 * kRad], m1[kRows + 2 * kRad], m2[kRows + 2 * kRad];
    auto load = [&](int r, float& a, float& b, float& c) __attribute__((always_inline)) {
        const bool in = has_ssim && col_in && r >= 0 && r < Hm;
        const size_t o = in ? (size_t)r * Wm + mcol : 0;
        a = in ? sv[o] : 0.0f;
        b = in ? sv[mp + o] : 0.0f;
        c = in ? sv[2 * mp + o] : 0.0f;
    };
    if (has_ssim) {
#pragma unroll
        for (int i = 0; i < 2 * kRad; ++i) load(y0 + shift + i, m0[i], m1[i], m2[i]);
    }

    for (int r0 = 0; r0 < kTileH; r0 += kRows) {
        if (y0 + r0 >= H) break;                             // (workgroup-uniform)
        if (has_ssim) {
#pragma unroll
            for (int i = 0; i < kRows; ++i)
                load(y0 + r0 + shift + 2 * kRad + i, m0[2 * kRad + i], m1[2 * kRad + i], m2[2 * kRad + i]);
#pragma unroll
            for (int o = 0; o < kRows; ++o) {
                float a = 0.0f, b = 0.0f, c = 0.0f;
#pragma unroll
                for (int k = 0; k < kTaps; ++k) {
                    a = fmaf(w[k], m0[o + k], a);
                    b = fmaf(w[k], m1[o + k], b);
                    c = fmaf(w[k], m2[o + k], c);
                }
                s_m[o][0][t] = a; s_m[o][1][t] = b; s_m[o][2][t] = c;
            }
            __syncthreads();
        }
        for (int it = t; it < kRows * kGroups; it += kThreads) {
            const int o = it / kGroups, c0 = 4 * (it - o * kGroups);
            const int yy = y0 + r0 + o;
            const int xx0 = x0 + c0;
            const int n = min(min(4, kTileW - c0), W - xx0);  // this group's pixels of the row: columns [xx0, xx0 + n)
            if (yy >= H || n <= 0) continue;
            float u[3][4];
            if (has_ssim) {
#pragma unroll
                for (int m = 0; m < 3; ++m) row_taps4(&s_m[o][m][c0], w, u[m]);
            }
            const size_t ro = base + (size_t)yy * W;
            float g[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                g[q] = 0.0f;
                if (q < n) {
                    const float p = pred[ro + xx0 + q], x = gt[ro + xx0 + q];
                    const float d = p - x;
                    float val = gl * (d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f));
                    if (has_ssim) {
                        // (identical images: u[1] == -2 u[0] and p == x, so the two products cancel exactly)
                        const float t1 = (2.0f * (p - kMid)) * u[0][q], t2 = (x - kMid) * u[1][q];
                        val += gs * (u[2][q] + (t1 + t2));
                    }
                    g[q] = val;
                }
            }
            store_row4(g_pred + ro, xx0, xx0 + n, g);
        }
        if (has_ssim) {
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 2 * kRad; ++i) { m0[i] = m0[kRows + i]; m1[i] = m1[kRows + i]; m2[i] = m2[kRows + i]; }
        }
    }
}

bool args_ok(int32_t B, int32_t C, int32_t H, int32_t W, int32_t flags)
{
    if (flags != FS_SSIM_SKIMAGE && flags != FS_SSIM_3DGS) return false;
    const int min_hw = flags == FS_SSIM_SKIMAGE ? kTaps : 1;
    if (B <= 0 || C <= 0 || H < min_hw || W < min_hw) return false;
    int tx, tiles;
    plane_tiles(H, W, tx, tiles);
    return (long long)B * C * tiles <= 0x7fffffffLL && (long long)H * W <= 0x7fffffffLL;
}

// averaged outputs per plane
long long outputs(int32_t H, int32_t W, int32_t flags)
{
    const int off = flags == FS_SSIM_SKIMAGE ? kRad : 0;
    return (long long)(H - 2 * off) * (W - 2 * off);
}

}  // namespace

}  // namespace fs

using namespace fs;

FS_API int fs_loss_api_version(void) { return FS_LOSS_API_VERSION; }

FS_API size_t fs_ssim_loss_saved_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t flags)
{
    if (!args_ok(B, C, H, W, flags)) return 0;
    return align_up((size_t)B * C * 3 * (size_t)outputs(H, W, flags) * sizeof(float), 256);
}

FS_API size_t fs_ssim_loss_scratch_bytes(int32_t B, int32_t C, int32_t H, int32_t W, int32_t flags)
{
    if (!args_ok(B, C, H, W, flags)) return 0;
    int tx, tiles;
    plane_tiles(H, W, tx, tiles);
    return align_up((size_t)B * C * tiles * sizeof(double2), 256);
}

FS_API int fs_ssim_loss_forward(int32_t B, int32_t C, int32_t H, int32_t W, int32_t flags, const float* pred, const float* gt,
                                double* ssim, double* l1_mean, void* saved, void* scratch, void* stream_)
{
    if (!args_ok(B, C, H, W, flags) || !pred || !gt || !ssim || !l1_mean || !scratch) return FS_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream_;
    int tiles_x, tiles;
    plane_tiles(H, W, tiles_x, tiles);
    const Weights wt = Weights::make();
    double2* rows = static_cast<double2*>(scratch);
    const dim3 grid((unsigned)(B * C * tiles));
    const bool pad = flags == FS_SSIM_3DGS;
    auto kernel = pad ? (saved ? ssim_loss_fwd_kernel<true, true> : ssim_loss_fwd_kernel<true, false>)
                      : (saved ? ssim_loss_fwd_kernel<false, true> : ssim_loss_fwd_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, st, H, W, tiles_x, tiles, pred, gt, wt, static_cast<float*>(saved), rows);
    const RowOuts<2> outs = {{ssim, l1_mean}, {1.0 / ((double)C * (double)outputs(H, W, flags)), 1.0 / ((double)C * H * W)}, 1};
    hipLaunchKernelGGL((finalize_rows_kernel<2, BlockSum::kTree, true>), dim3((unsigned)B), dim3(kThreads), 0, st, C * tiles, 1,
                       reinterpret_cast<const double*>(rows), outs);
    FS_CHECK_LAUNCH("ssim_loss_forward");
    return FS_OK;
}

FS_API int fs_ssim_loss_backward(int32_t B, int32_t C, int32_t H, int32_t W, int32_t flags, const float* pred, const float* gt,
                                 const float* g_ssim, const float* g_l1, const void* saved, float* g_pred, void* scratch,
                                 void* stream_)
{
    (void)scratch;                                           // reserved
    if (!args_ok(B, C, H, W, flags) || !pred || !gt || !g_pred || (!g_ssim && !g_l1) || (g_ssim && !saved))
        return FS_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream_;
    int tiles_x, tiles;
    plane_tiles(H, W, tiles_x, tiles);
    const Weights wt = Weights::make();
    const float scale_ssim = (float)(1.0 / ((double)C * (double)outputs(H, W, flags)));
    const float scale_l1 = (float)(1.0 / ((double)C * H * W));
    const dim3 grid((unsigned)(B * C * tiles));
    if (flags == FS_SSIM_3DGS)
        hipLaunchKernelGGL(ssim_loss_bwd_kernel<true>, grid, dim3(kThreads), 0, st, C, H, W, tiles_x, tiles, pred, gt, g_ssim, g_l1,
                           static_cast<const float*>(saved), scale_ssim, scale_l1, wt, g_pred);
    else
        hipLaunchKernelGGL(ssim_loss_bwd_kernel<false>, grid, dim3(kThreads), 0, st, C, H, W, tiles_x, tiles, pred, gt, g_ssim,
                           g_l1, static_cast<const float*>(saved), scale_ssim, scale_l1, wt, g_pred);
    FS_CHECK_LAUNCH("ssim_loss_backward");
    return FS_OK;
}
