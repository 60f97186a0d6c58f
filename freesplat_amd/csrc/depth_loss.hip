// depth_loss.hip -- depth-supervision loss (include/freesplat_amd_depthloss.h): a log-L1 / L1 point term and a multi-scale
// Sobel gradient term over a blur-pool pyramid, forward and backward.
//
// Every step of the gradient term is linear, so ONE pyramid is built, of the residual R = E - gt, and an invalid element is
// stored as NaN: the blur pool has no zero weight, so plain arithmetic carries validity from level to level ("every tap
// inside the level is valid"); the Sobel sum tests its nine taps explicitly (its centre weights are zero).  An invalid gt is
// never read into arithmetic: the residual of such a pixel is the constant NaN.
//
// Forward: one launch per level.  A workgroup owns kTileW x kTileH elements of level 0 (kTileW x kUpperTileH of a level above), loads them with a halo of 1
// (replicate-clamped coordinates, which is what the Sobel taps want) into LDS, adds the level's gradient term and, for level
// 0, the point term while the pixel passes through registers, and writes its (kTileW/2) x (kTileH/2) elements of the next
// level (taps outside the level contribute 0).  Level 0 reads depth, gt and alpha (12 B per pixel); levels 1.. read the
// level below from the pyramid buffer (`saved` when a backward is pending, otherwise scratch): 4/3 B per level-0 pixel
// written and read once more.
//
// Backward: one launch per level, from the top down; a gather.  A workgroup owns the same tile of its level, loads
// the residual with a halo of 2, forms the signs of g_x and g_y of the outputs with a halo of 1 in LDS, and every element
// collects the (at most nine) Sobel outputs that read it -- the replicate clamp folds into two extra 1-D weights at the
// borders -- and the (at most four) elements of the level above whose blur-pool window holds it.  Level 0 recomputes its
// residual from depth, gt and alpha and applies dE/d depth, dE/d alpha and the point term.  Every output element is written
// by exactly one thread; nothing is accumulated in memory.
//
// Deterministic: per-thread sums in a fixed order, block_sum_tree (fs_reduce.h) per workgroup, one partial row per workgroup, a
// finalize workgroup per (view, level).  The partition depends only on (H, W, S).  No atomics.
#include "fs_reduce.h"

#include "../../include/freesplat_amd_depthloss.h"

namespace fs {

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 64;                    // elements of a level per workgroup: kTileW x kTileH at level 0 (freesplat_amd/
constexpr int kTileH = 32;                    // depth_loss.py TILE_W, TILE_H), kTileW x kUpperTileH at levels 1.. (UPPER_TILE_H):
constexpr int kUpperTileH = 8;                // those grids are small, and a thread with 2 elements finishes 4x sooner than one with 8
constexpr int kMaxS = FS_DEPTH_LOSS_MAX_SCALES;

// extents that follow from the tile height TH: forward patch (halo 1), backward patch (halo 2) and sign maps (halo 1),
// patch / tile elements per thread
template <int TH>
struct Tile {
    static constexpr int kFwdW = kTileW + 2, kFwdH = TH + 2;
    static constexpr int kBwdW = kTileW + 4, kBwdH = TH + 4;
    static constexpr int kSgnW = kTileW + 2, kSgnH = TH + 2;
    static constexpr int kFwdIters = (kFwdH * kFwdW + kThreads - 1) / kThreads;
    static constexpr int kBwdIters = (kBwdH * kBwdW + kThreads - 1) / kThreads;
    static constexpr int kTileIters = TH * kTileW / kThreads;
    static_assert(TH * kTileW % kThreads == 0 && TH % 2 == 0 && kTileW % 2 == 0, "tile / workgroup shape");
};

struct Params {
    int mode;
    float min_depth, max_depth, alpha_floor;
};

struct Row {                                  // one workgroup's partial sums
    double point_sum, point_cnt, grad_sum, grad_cnt;
};

__device__ __forceinline__ float sgn(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }

// level-0 pixel from its raw values: expected depth E, the gt value (0 when invalid) and the residual (NaN when invalid)
__device__ __forceinline__ float residual0(float d, float graw, float al, bool has_alpha, const Params& P, float& E, float& g,
                                           bool& valid)
{
    valid = valid_depth(graw, P.min_depth, P.max_depth);
    g = valid ? graw : 0.0f;
    E = expected_depth<float>(d, al, has_alpha, P.alpha_floor);
    return valid ? E - g : __builtin_nanf("");
}

// the two Sobel sums (x8) of the 3 x 3 patch whose top-left element is p[0], rows `stride` apart; false: a tap is invalid
__device__ __forceinline__ bool sobel(const float* p, int stride, float& gx, float& gy)
{
    const float a00 = p[0], a01 = p[1], a02 = p[2];
    const float a10 = p[stride], a11 = p[stride + 1], a12 = p[stride + 2];
    const float a20 = p[2 * stride], a21 = p[2 * stride + 1], a22 = p[2 * stride + 2];
    gx = ((a02 - a00) + (a22 - a20)) + 2.0f * (a12 - a10);
    gy = ((a20 - a00) + (a22 - a02)) + 2.0f * (a21 - a01);
    const float all = (gx + gy) + a11;                   // NaN iff one of the nine taps is NaN (the inputs are finite)
    return all == all;
}

// One tile of level s of one view.  blockIdx.x = view * tiles + tile.  L0: src = depth (with gt, alpha), else src = level s of
// the pyramid.  next: NULL (s is the top level) or level s + 1 [views][Hn][Wn].  rows[blockIdx.x] receives the partial sums.
template <bool L0, int TH>
__global__ __launch_bounds__(kThreads) void depth_loss_fwd_kernel(int Hs, int Ws, int tiles_x, int tiles,
                                                                  const float* __restrict__ src, const float* __restrict__ gt,
                                                                  const float* __restrict__ alpha, Params P, int Hn, int Wn,
                                                                  float* __restrict__ next, Row* __restrict__ rows)
{
    constexpr int kTileH = TH, kFwdH = Tile<TH>::kFwdH, kFwdW = Tile<TH>::kFwdW, kFwdIters = Tile<TH>::kFwdIters;
    __shared__ float s_r[kFwdH][kFwdW];
    __shared__ double s_red[4 * kThreads];
    const int t = threadIdx.x;
    const long long view = blockIdx.x / tiles;
    const int tile = blockIdx.x - (int)(view * tiles);
    const int x0 = (tile % tiles_x) * kTileW, y0 = (tile / tiles_x) * kTileH;
    const size_t base = (size_t)view * Hs * Ws;
    double p_sum = 0.0, g_sum = 0.0;
    int p_cnt = 0, g_cnt = 0;

    // every load of the patch is issued before the first value is used (kFwdIters independent loads per array and thread);
    // a slot past the patch reads a clamped, in-range address and is dropped
    float v_src[kFwdIters], v_gt[kFwdIters], v_al[kFwdIters];
#pragma unroll
    for (int k = 0; k < kFwdIters; ++k) {
        const int i = t + k * kThreads;
        const int ly = i / kFwdW, lx = i - ly * kFwdW;
        const int yc = min(max(y0 - 1 + ly, 0), Hs - 1), xc = min(max(x0 - 1 + lx, 0), Ws - 1);
        const size_t o = base + (size_t)yc * Ws + xc;
        v_src[k] = src[o];
        if constexpr (L0) {
            v_gt[k] = gt[o];
            v_al[k] = alpha ? alpha[o] : 1.0f;
        }
    }
#pragma unroll
    for (int k = 0; k < kFwdIters; ++k) {
        const int i = t + k * kThreads;
        const int ly = i / kFwdW, lx = i - ly * kFwdW;
        if (ly >= kFwdH) continue;
        const int y = y0 - 1 + ly, x = x0 - 1 + lx;
        float r = v_src[k];
        if constexpr (L0) {
            float E, g;
            bool valid;
            r = residual0(v_src[k], v_gt[k], v_al[k], alpha != nullptr, P, E, g, valid);
            const bool own = y >= 0 && y < Hs && x >= 0 && x < Ws && ly >= 1 && ly <= kTileH && lx >= 1 && lx <= kTileW;
            if (own && valid) {
                if (P.mode == FS_DEPTH_LOSS_LOG_L1) {
                    if (E > 0.0f) {
                        p_sum += (double)fabsf(__logf(E / g));          // log E - log gt: one division, one v_log_f32
                        ++p_cnt;
                    }
                } else {
                    p_sum += (double)fabsf(r);
                    ++p_cnt;
                }
            }
        }
        s_r[ly][lx] = r;
    }
    __syncthreads();

    // the level's gradient term
    for (int i = t; i < kTileH * kTileW; i += kThreads) {
        const int ly = i / kTileW, lx = i - ly * kTileW;
        if (y0 + ly >= Hs || x0 + lx >= Ws) continue;
        float gx, gy;
        if (sobel(&s_r[ly][lx], kFwdW, gx, gy)) {
            g_sum += (double)(0.125f * (fabsf(gx) + fabsf(gy)));
            g_cnt += 2;
        }
    }

    // the next level's elements: rows 2 Y - 1 .. 2 Y + 1 of this level, those outside it left out
    if (next) {
        const int Y0 = y0 / 2, X0 = x0 / 2;
        for (int i = t; i < (kTileH / 2) * (kTileW / 2); i += kThreads) {
            const int oy = i / (kTileW / 2), ox = i - oy * (kTileW / 2);
            const int Y = Y0 + oy, X = X0 + ox;
            if (Y >= Hn || X >= Wn) continue;
            float acc = 0.0f;
#pragma unroll
            for (int a = -1; a <= 1; ++a) {
                const int yy = 2 * Y + a;
                if (yy < 0 || yy >= Hs) continue;
                float row = 0.0f;
#pragma unroll
                for (int b = -1; b <= 1; ++b) {
                    const int xx = 2 * X + b;
                    if (xx < 0 || xx >= Ws) continue;
                    const float v = s_r[yy - y0 + 1][xx - x0 + 1];
                    row += b == 0 ? 2.0f * v : v;
                }
                acc += a == 0 ? 2.0f * row : row;
            }
            next[(size_t)view * Hn * Wn + (size_t)Y * Wn + X] = 0.0625f * acc;
        }
    }

    double v[4] = {p_sum, (double)p_cnt, g_sum, (double)g_cnt};
    block_sum_tree<4>(v, s_red);
    if (t == 0) rows[blockIdx.x] = Row{v[0], v[1], v[2], v[3]};
}

struct Levels {
    int H[kMaxS], W[kMaxS], tiles_x[kMaxS], tiles[kMaxS];
    long long row_off[kMaxS];                // first partial row of level s (rows of a level: [view][tile])
    long long pyr_off[kMaxS];                // first float of level s in the pyramid buffer (s >= 1)
    long long n_rows, n_pyr;
};

// one workgroup per (view, level): the view's partial rows of that level in a fixed order
__global__ __launch_bounds__(kThreads) void depth_loss_finalize_kernel(int S, Levels lv, const Row* __restrict__ rows,
                                                                       double* __restrict__ point_sum, double* __restrict__ point_cnt,
                                                                       double* __restrict__ grad_sum, double* __restrict__ grad_cnt)
{
    __shared__ double s_red[4 * kThreads];
    const int view = blockIdx.x / S, s = blockIdx.x - view * S;
    const int K = lv.tiles[s];
    const Row* r = rows + lv.row_off[s] + (long long)view * K;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < K; k += kThreads) {
        v[0] += r[k].point_sum;
        v[1] += r[k].point_cnt;
        v[2] += r[k].grad_sum;
        v[3] += r[k].grad_cnt;
    }
    block_sum_tree<4>(v, s_red);
    if (threadIdx.x == 0) {
        grad_sum[blockIdx.x] = v[2];
        grad_cnt[blockIdx.x] = v[3];
        if (s == 0) {
            point_sum[view] = v[0];
            point_cnt[view] = v[1];
        }
    }
}

// One tile of level s of one view, backward.  L0: src = depth (with gt, alpha) and out = g_depth (with g_alpha), else src =
// level s of the saved pyramid and out = level s of the cotangent pyramid.  up: NULL or the cotangent of level s + 1
// [views][Hn][Wn].  g_grad: NULL (no gradient term: src is then read only for the point term) or [views][S].
template <bool L0, int TH>
__global__ __launch_bounds__(kThreads) void depth_loss_bwd_kernel(int S, int s, int Hs, int Ws, int tiles_x, int tiles,
                                                                  const float* __restrict__ src, const float* __restrict__ gt,
                                                                  const float* __restrict__ alpha, Params P,
                                                                  const float* __restrict__ g_point, const float* __restrict__ g_grad,
                                                                  int Hn, int Wn, const float* __restrict__ up,
                                                                  float* __restrict__ out, float* __restrict__ g_alpha)
{
    constexpr int kTileH = TH, kBwdH = Tile<TH>::kBwdH, kBwdW = Tile<TH>::kBwdW, kSgnH = Tile<TH>::kSgnH, kSgnW = Tile<TH>::kSgnW;
    constexpr int kBwdIters = Tile<TH>::kBwdIters, kTileIters = Tile<TH>::kTileIters;
    __shared__ float s_r[kBwdH][kBwdW];
    __shared__ float s_cx[kSgnH][kSgnW], s_cy[kSgnH][kSgnW];
    const int t = threadIdx.x;
    const long long view = blockIdx.x / tiles;
    const int tile = blockIdx.x - (int)(view * tiles);
    const int x0 = (tile % tiles_x) * kTileW, y0 = (tile / tiles_x) * kTileH;
    const size_t base = (size_t)view * Hs * Ws;
    const bool has_grad = g_grad != nullptr;                 // (kernel-uniform)
    const float coef = has_grad ? 0.125f * g_grad[view * S + s] : 0.0f;

    // level 0: the thread's own pixels (element k of the tile loop below), loaded before anything waits
    float own_d[kTileIters], own_g[kTileIters], own_a[kTileIters];
    if constexpr (L0) {
#pragma unroll
        for (int k = 0; k < kTileIters; ++k) {
            const int i = t + k * kThreads;
            const int yc = min(y0 + i / kTileW, Hs - 1), xc = min(x0 + i % kTileW, Ws - 1);
            const size_t o = base + (size_t)yc * Ws + xc;
            own_d[k] = src[o];
            own_g[k] = gt[o];
            own_a[k] = alpha ? alpha[o] : 1.0f;
        }
    }

    // the level above: the (at most four) elements (qy, qx) with 2 q + a = p for a tap a in -1..1, again loaded up front
    float from_up[kTileIters];
#pragma unroll
    for (int k = 0; k < kTileIters; ++k) {
        from_up[k] = 0.0f;
        if (!has_grad || !up) continue;
        const int i = t + k * kThreads;
        const int y = y0 + i / kTileW, x = x0 + i % kTileW;
        if (y >= Hs || x >= Ws) continue;
        float u = 0.0f;
#pragma unroll
        for (int a = -1; a <= 1; ++a) {
            const int ty = y - a;
            if (ty < 0 || (ty & 1) || (ty >> 1) >= Hn) continue;
            float row = 0.0f;
#pragma unroll
            for (int b = -1; b <= 1; ++b) {
                const int tx = x - b;
                if (tx < 0 || (tx & 1) || (tx >> 1) >= Wn) continue;
                const float v = up[(size_t)view * Hn * Wn + (size_t)(ty >> 1) * Wn + (tx >> 1)];
                row += b == 0 ? 2.0f * v : v;
            }
            u += a == 0 ? 2.0f * row : row;
        }
        from_up[k] = 0.0625f * u;
    }

    if (has_grad) {
        float v_src[kBwdIters], v_gt[kBwdIters], v_al[kBwdIters];
#pragma unroll
        for (int k = 0; k < kBwdIters; ++k) {
            const int i = t + k * kThreads;
            const int ly = i / kBwdW, lx = i - ly * kBwdW;
            const int yc = min(max(y0 - 2 + ly, 0), Hs - 1), xc = min(max(x0 - 2 + lx, 0), Ws - 1);
            const size_t o = base + (size_t)yc * Ws + xc;
            v_src[k] = src[o];
            if constexpr (L0) {
                v_gt[k] = gt[o];
                v_al[k] = alpha ? alpha[o] : 1.0f;
            }
        }
#pragma unroll
        for (int k = 0; k < kBwdIters; ++k) {
            const int i = t + k * kThreads;
            const int ly = i / kBwdW, lx = i - ly * kBwdW;
            if (ly >= kBwdH) continue;
            float r = v_src[k];
            if constexpr (L0) {
                float E, g;
                bool valid;
                r = residual0(v_src[k], v_gt[k], v_al[k], alpha != nullptr, P, E, g, valid);
            }
            s_r[ly][lx] = r;
        }
        __syncthreads();
        // signs of g_x, g_y of the outputs (y0 - 1 + ly, x0 - 1 + lx); 0 outside the level and where a tap is invalid
        for (int i = t; i < kSgnH * kSgnW; i += kThreads) {
            const int ly = i / kSgnW, lx = i - ly * kSgnW;
            const int y = y0 - 1 + ly, x = x0 - 1 + lx;
            float cx = 0.0f, cy = 0.0f;
            if (y >= 0 && y < Hs && x >= 0 && x < Ws) {
                float gx, gy;
                if (sobel(&s_r[ly][lx], kBwdW, gx, gy)) {
                    cx = sgn(gx);
                    cy = sgn(gy);
                }
            }
            s_cx[ly][lx] = cx;
            s_cy[ly][lx] = cy;
        }
        __syncthreads();
    }

#pragma unroll
    for (int k = 0; k < kTileIters; ++k) {
        const int i = t + k * kThreads;
        const int ly = i / kTileW, lx = i - ly * kTileW;
        const int y = y0 + ly, x = x0 + lx;
        if (y >= Hs || x >= Ws) continue;
        float G = 0.0f;
        if (has_grad) {
            // 1-D weights of the outputs p - 1, p, p + 1 on element p: the smoothing taps (1, 2, 1) and the difference taps
            // (-1, 0, 1) that land on p, the clamped ones of the border outputs included
            const float lo_y = y == 0 ? 1.0f : 0.0f, hi_y = y == Hs - 1 ? 1.0f : 0.0f;
            const float lo_x = x == 0 ? 1.0f : 0.0f, hi_x = x == Ws - 1 ? 1.0f : 0.0f;
            const float wsy[3] = {1.0f, 2.0f + lo_y + hi_y, 1.0f}, wdy[3] = {1.0f, hi_y - lo_y, -1.0f};
            const float wsx[3] = {1.0f, 2.0f + lo_x + hi_x, 1.0f}, wdx[3] = {1.0f, hi_x - lo_x, -1.0f};
            float acc = 0.0f;                                // (small integers: exact)
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b)
                    acc += wsy[a] * wdx[b] * s_cx[ly + a][lx + b] + wdy[a] * wsx[b] * s_cy[ly + a][lx + b];
            G = coef * acc + from_up[k];
        }
        const size_t o = base + (size_t)y * Ws + x;
        if constexpr (!L0) {
            out[o] = G;
        } else {
            float E, g;
            bool valid;
            const float r = residual0(own_d[k], own_g[k], own_a[k], alpha != nullptr, P, E, g, valid);
            float gd = 0.0f, ga = 0.0f;
            if (valid) {
                float dE = G;
                if (g_point) {
                    const float gp = g_point[view];
                    if (P.mode == FS_DEPTH_LOSS_LOG_L1) {
                        if (E > 0.0f) dE += gp * sgn(r) / E;                // sign(log E - log gt) = sign(E - gt)
                    } else {
                        dE += gp * sgn(r);
                    }
                }
                if (alpha) {
                    const float al = own_a[k];
                    gd = dE / fmaxf(al, P.alpha_floor);
                    ga = al > P.alpha_floor ? -(gd * E) : 0.0f;         // -dE E / alpha, max(alpha, floor) = alpha here
                } else {
                    gd = dE;
                }
            }
            out[o] = gd;
            if (alpha) g_alpha[o] = ga;
        }
    }
}

bool make_levels(int32_t B, int32_t H, int32_t W, int32_t S, Levels& lv)
{
    if (B <= 0 || H <= 0 || W <= 0 || S < 1 || S > kMaxS) return false;
    if ((long long)H * W > 0x7fffffffLL) return false;
    lv.n_rows = 0;
    lv.n_pyr = 0;
    for (int s = 0; s < kMaxS; ++s) {
        lv.H[s] = lv.W[s] = lv.tiles_x[s] = lv.tiles[s] = 0;
        lv.row_off[s] = lv.pyr_off[s] = 0;
    }
    int h = H, w = W;
    for (int s = 0; s < S; ++s) {
        lv.H[s] = h;
        lv.W[s] = w;
        lv.tiles_x[s] = (w + kTileW - 1) / kTileW;
        const int th = s == 0 ? kTileH : kUpperTileH;
        lv.tiles[s] = lv.tiles_x[s] * ((h + th - 1) / th);
        if ((long long)B * lv.tiles[s] > 0x7fffffffLL) return false;
        lv.row_off[s] = lv.n_rows;
        lv.n_rows += (long long)B * lv.tiles[s];
        if (s >= 1) {
            lv.pyr_off[s] = lv.n_pyr;
            lv.n_pyr += (long long)B * h * w;
        }
        h = (h + 1) / 2;
        w = (w + 1) / 2;
    }
    return true;
}

bool scalars_ok(int32_t mode, float min_depth, float max_depth, float alpha_floor)
{
    if (mode != FS_DEPTH_LOSS_LOG_L1 && mode != FS_DEPTH_LOSS_L1) return false;
    if (min_depth != min_depth || max_depth != max_depth) return false;
    return alpha_floor > 0.0f && alpha_floor < INFINITY;
}

size_t rows_bytes(const Levels& lv) { return align_up((size_t)lv.n_rows * sizeof(Row), 256); }
size_t pyr_bytes(const Levels& lv) { return align_up((size_t)(lv.n_pyr > 0 ? lv.n_pyr : 1) * sizeof(float), 256); }

}  // namespace

}  // namespace fs

using namespace fs;

FS_API int fs_depthloss_api_version(void) { return FS_DEPTHLOSS_API_VERSION; }

FS_API size_t fs_depth_loss_saved_bytes(int32_t B, int32_t H, int32_t W, int32_t S)
{
    Levels lv;
    if (!make_levels(B, H, W, S, lv)) return 0;
    return pyr_bytes(lv);
}

FS_API size_t fs_depth_loss_scratch_bytes(int32_t B, int32_t H, int32_t W, int32_t S)
{
    Levels lv;
    if (!make_levels(B, H, W, S, lv)) return 0;
    return rows_bytes(lv) + pyr_bytes(lv);                   // forward: partial rows + the pyramid; backward: the cotangent pyramid
}

FS_API int fs_depth_loss_forward(int32_t B, int32_t H, int32_t W, int32_t S, int32_t mode, const float* depth, const float* gt,
                                 const float* alpha, float min_depth, float max_depth, float alpha_floor, double* point_sum,
                                 double* point_cnt, double* grad_sum, double* grad_cnt, void* saved, void* scratch, void* stream_)
{
    Levels lv;
    if (!make_levels(B, H, W, S, lv) || !scalars_ok(mode, min_depth, max_depth, alpha_floor) || !depth || !gt || !point_sum ||
        !point_cnt || !grad_sum || !grad_cnt || !scratch)
        return FS_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream_;
    const Params P{mode, min_depth, max_depth, alpha_floor};
    Row* rows = static_cast<Row*>(scratch);
    float* pyr = saved ? static_cast<float*>(saved) : reinterpret_cast<float*>(static_cast<char*>(scratch) + rows_bytes(lv));
    for (int s = 0; s < S; ++s) {
        const bool top = s + 1 == S;
        float* next = top ? nullptr : pyr + lv.pyr_off[s + 1];
        const int Hn = top ? 0 : lv.H[s + 1], Wn = top ? 0 : lv.W[s + 1];
        const dim3 grid((unsigned)(B * lv.tiles[s]));
        if (s == 0)
            hipLaunchKernelGGL((depth_loss_fwd_kernel<true, kTileH>), grid, dim3(kThreads), 0, st, H, W, lv.tiles_x[0], lv.tiles[0], depth, gt,
                               alpha, P, Hn, Wn, next, rows);
        else
            hipLaunchKernelGGL((depth_loss_fwd_kernel<false, kUpperTileH>), grid, dim3(kThreads), 0, st, lv.H[s], lv.W[s], lv.tiles_x[s],
                               lv.tiles[s], (const float*)(pyr + lv.pyr_off[s]), (const float*)nullptr, (const float*)nullptr, P,
                               Hn, Wn, next, rows + lv.row_off[s]);
    }
    hipLaunchKernelGGL(depth_loss_finalize_kernel, dim3((unsigned)(B * S)), dim3(kThreads), 0, st, S, lv, (const Row*)rows,
                       point_sum, point_cnt, grad_sum, grad_cnt);
    FS_CHECK_LAUNCH("depth_loss_forward");
    return FS_OK;
}

FS_API int fs_depth_loss_backward(int32_t B, int32_t H, int32_t W, int32_t S, int32_t mode, const float* depth, const float* gt,
                                  const float* alpha, float min_depth, float max_depth, float alpha_floor, const float* g_point,
                                  const float* g_grad, const void* saved, float* g_depth, float* g_alpha, void* scratch,
                                  void* stream_)
{
    Levels lv;
    if (!make_levels(B, H, W, S, lv) || !scalars_ok(mode, min_depth, max_depth, alpha_floor) || !depth || !gt || !g_depth ||
        (alpha && !g_alpha) || (!g_point && !g_grad) || (g_grad && (!saved || !scratch)))
        return FS_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream_;
    const Params P{mode, min_depth, max_depth, alpha_floor};
    const float* pyr = static_cast<const float*>(saved);
    float* cot = static_cast<float*>(scratch);               // cotangents of levels 1 .. S - 1, laid out as the pyramid
    if (g_grad)
        for (int s = S - 1; s >= 1; --s) {
            const bool top = s + 1 == S;
            hipLaunchKernelGGL((depth_loss_bwd_kernel<false, kUpperTileH>), dim3((unsigned)(B * lv.tiles[s])), dim3(kThreads), 0, st, S, s, lv.H[s],
                               lv.W[s], lv.tiles_x[s], lv.tiles[s], pyr + lv.pyr_off[s], (const float*)nullptr,
                               (const float*)nullptr, P, (const float*)nullptr, g_grad, top ? 0 : lv.H[s + 1],
                               top ? 0 : lv.W[s + 1], top ? (const float*)nullptr : (const float*)(cot + lv.pyr_off[s + 1]),
                               cot + lv.pyr_off[s], (float*)nullptr);
        }
    const bool has_up = g_grad && S > 1;
    hipLaunchKernelGGL((depth_loss_bwd_kernel<true, kTileH>), dim3((unsigned)(B * lv.tiles[0])), dim3(kThreads), 0, st, S, 0, H, W,
                       lv.tiles_x[0], lv.tiles[0], depth, gt, alpha, P, g_point, g_grad, has_up ? lv.H[1] : 0, has_up ? lv.W[1] : 0,
                       has_up ? (const float*)(cot + lv.pyr_off[1]) : (const float*)nullptr, g_depth, g_alpha);
    FS_CHECK_LAUNCH("depth_loss_backward");
    return FS_OK;
}
