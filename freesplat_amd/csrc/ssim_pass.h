// ssim_pass.h -- what the tiled SSIM kernels share: metrics.hip's ssim_tile_kernel and ssim_loss.hip's forward and backward.
// The constants, the Gaussian weights and the pieces of the two passes live here; the kernels keep their own bodies.
//
// A workgroup of 256 threads owns kTileW x kTileH pixels of one (view, channel) plane:
//   vertical 11-tap pass: one thread per patch column (kTileW + 10 = 256) sliding down the rows with the inputs of the last
//     10 + kRows rows in registers; the five moments x, y, x^2, y^2, xy of kRows rows go to LDS (column_moments);
//   horizontal 11-tap pass: a thread takes 4 consecutive outputs of a row (16-byte LDS reads, row_taps4), forms S
//     (ssim_terms) and adds it to its partial when the output is one the convention averages.
#pragma once
#include "fs_reduce.h"

namespace fs {

namespace ssim {

constexpr int kRad = 5;                           // sigma 1.5, truncate 3.5: int(3.5 * 1.5 + 0.5)
constexpr int kTaps = 2 * kRad + 1;
constexpr int kTileW = kSumThreads - 2 * kRad;    // 246 columns per workgroup: patch column = thread
constexpr int kTileH = 64;                        // rows per workgroup
constexpr int kRows = 8;                          // rows per LDS round
constexpr int kGroups = (kTileW + 3) / 4;         // 62 groups of 4 columns in the horizontal pass
constexpr int kLdsRow = 260;                      // >= 4 * (kGroups - 1) + 16: the last group's 16-byte reads stay in the row
constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;
constexpr float kMid = 0.5f;                      // the saved G*y map and the backward's pred / gt factors are taken about this

struct Weights {
    float w[kTaps];
    // Gaussian weights as scipy.ndimage builds them: exp(-k^2 / (2 sigma^2)) normalised in double, k = -5..5
    static Weights make()
    {
        Weights wt;
        double e[kTaps], sum = 0.0;
        for (int k = 0; k < kTaps; ++k) {
            const double d = k - kRad;
            e[k] = exp(-0.5 * d * d / (1.5 * 1.5));
            sum += e[k];
        }
        for (int k = 0; k < kTaps; ++k) wt.w[k] = (float)(e[k] / sum);
        return wt;
    }
};

inline void plane_tiles(int H, int W, int& tiles_x, int& tiles)
{
    tiles_x = (W + kTileW - 1) / kTileW;
    tiles = tiles_x * ((H + kTileH - 1) / kTileH);
}

// A tile's moments are taken about a pivot, the value of its first pixel in each image (0.5 where that is not finite or lies
// outside [-1, 2]): that keeps u_xx - u_x^2 from cancelling away the variance of smooth images (4 - 8x smaller per-pixel error
// than raw values) and makes every variance of a constant image exactly 0.
__device__ __forceinline__ float pivot_of(float v) { return v >= -1.0f && v <= 2.0f ? v : 0.5f; }

// vertical pass of one output row of a column: the moments x, y, x^2, y^2, xy of the 11 centred inputs at x, y.  The x- and
// y-terms take identical operation sequences (identical images give S = 1 exactly).
__device__ __forceinline__ void column_moments(const float* x_, const float* y_, const float (&w)[kTaps], float (&m)[5])
{
    float ux = 0.0f, uy = 0.0f, uxx = 0.0f, uyy = 0.0f, uxy = 0.0f;
#pragma unroll
    for (int k = 0; k < kTaps; ++k) {
        const float x = x_[k], y = y_[k];
        const float wx = w[k] * x, wy = w[k] * y;
        ux += wx;
        uy += wy;
        uxx = fmaf(wx, x, uxx);
        uyy = fmaf(wy, y, uyy);
        uxy = fmaf(wx, y, uxy);
    }
    m[0] = ux; m[1] = uy; m[2] = uxx; m[3] = uyy; m[4] = uxy;
}

// S = (a1 a2) / (b1 b2) of one output from its five filtered moments about the pivots (ox, oy); kF: NP / (NP - 1) for the sample
// covariance, 1 for the population covariance
struct Terms {
    float cx, cy, ux, uy, a1, a2, b1, b2, S;
};
__device__ __forceinline__ Terms ssim_terms(float cx, float cy, float uxx, float uyy, float uxy, float ox, float oy, float kF)
{
    Terms r;
    r.cx = cx; r.cy = cy;                                    // (means of the centred values)
    const float vx = kF * (uxx - cx * cx);
    const float vy = kF * (uyy - cy * cy);
    const float vxy = kF * (uxy - cx * cy);
    r.ux = cx + ox; r.uy = cy + oy;
    r.a1 = 2.0f * (r.ux * r.uy) + kC1; r.a2 = 2.0f * vxy + kC2;
    r.b1 = (r.ux * r.ux + r.uy * r.uy) + kC1; r.b2 = (vx + vy) + kC2;
    r.S = (r.a1 * r.a2) / (r.b1 * r.b2);
    return r;
}

// the 11-tap sums of 4 consecutive outputs from the 16 floats at `row` (16-byte aligned LDS)
__device__ __forceinline__ void row_taps4(const float* row, const float (&w)[kTaps], float (&u)[4])
{
    float v[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 f = *reinterpret_cast<const float4*>(row + 4 * q);
        v[4 * q] = f.x; v[4 * q + 1] = f.y; v[4 * q + 2] = f.z; v[4 * q + 3] = f.w;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float a = 0.0f;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) a = fmaf(w[k], v[q + k], a);
        u[q] = a;
    }
}

// 4 consecutive floats of a row: one 16-byte store where the address allows it and all four belong to the row
__device__ __forceinline__ void store_row4(float* __restrict__ row, int col, int n_cols, const float (&v)[4])
{
    float* p = row + col;
    if (col + 3 < n_cols && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (col + q < n_cols) p[q] = v[q];
    }
}

}  // namespace ssim

}  // namespace fs
