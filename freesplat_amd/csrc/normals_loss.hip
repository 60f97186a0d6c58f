// normals_loss.hip -- surface normals from depth and the cosine normals loss (include/freesplat_amd_normals.h), forward and
// backward.  The chain is depth -> (5 x 5 blur) -> camera-space points -> Sobel / 8 -> cross product -> normalise, applied to
// the predicted depth and, when the target is a depth map, to the target as well.
//
// An invalid depth is stored as NaN.  The blur has no zero weight, so plain arithmetic carries validity through it ("all 25
// clamped taps are valid"); the Sobel sums have zero centre weights, so a normal tests its nine taps explicitly.  Every map in
// LDS holds, at every position of its patch, the value of the replicate-CLAMPED coordinate: a tap is then read at its plain
// offset, and only the centre of a blur window is clamped by hand.
//
// Forward: a workgroup owns kTileW x kTileH pixels, loads the depth (and the target depth) with a halo of 3 (blur 2 + Sobel 1;
// 1 without smoothing) into LDS, runs the blur separably and forms its pixels' normals from LDS.  The loss form never writes a
// normal: the pixel's 0.5 (1 - n . t) goes into the thread's fp64 sum, block_sum_tree (fs_reduce.h) gives one partial row per
// workgroup, finalize_rows_kernel adds a view's rows.  The partition depends only on (H, W).  No float atomics (the one LDS
// atomic is an integer min, whose result does not depend on the order).
//
// Arithmetic: fp32 up to the two Sobel vectors, with the depth patch carried relative to its smallest valid depth
// (build_map()), fp64 from the cross product on (normal_at()): both because the quantities cancel.
//
// Backward: a gather; everything is recomputed from the inputs.  The workgroup rebuilds the smoothed depth on a halo of 4
// (from the depth on a halo of 6), forms for every pixel q of a halo-3 region the cotangents of its two Sobel vectors
// (normalise Jacobian, then Gy x . and . x Gx), six floats per pixel in LDS; every pixel p of a halo-2 region collects the (at
// most nine) Sobel outputs that read it -- the replicate clamp folds into 1-D weights at the borders -- and dots the result
// with its own ray: the cotangent of S; every tile pixel then collects the (at most 25) blur outputs that read it, the clamp
// again folded into 1-D weights, and applies dE / d depth and dE / d alpha.  Without smoothing the halos are 2 / 1 / 0 and
// the last step falls away (an instantiation of its own).  Every output element is written by exactly one thread.
#include "fs_reduce.h"

#include "../../include/freesplat_amd_normals.h"

namespace fs {

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 32;                    // pixels per workgroup (freesplat_amd/normals_loss.py TILE_W, TILE_H): two per
constexpr int kTileH = 16;                    // thread; the backward's LDS (36.3 KiB with smoothing) admits 4 workgroups per CU
constexpr float kNormEps = 1e-12f;            // F.normalize's floor on |Gx x Gy|

enum Mode { kGtDepth = 0, kGtNormals = 1, kMap = 2 };     // target from a depth map, target given, or the normal map itself

// extents that follow from the smoothing and from RN, the halo on which normals are needed (0 forward; 3 or 1 backward)
template <bool SMOOTH, int RN>
struct Geo {
    static constexpr int kB = SMOOTH ? 2 : 0;                                   // blur radius
    static constexpr int kHS = RN + 1, kHE = kHS + kB;                          // halo of S (Sobel taps) and of E (blur taps)
    static constexpr int kEW = kTileW + 2 * kHE, kEH = kTileH + 2 * kHE;        // depth patch
    static constexpr int kSW = kTileW + 2 * kHS, kSH = kTileH + 2 * kHS;        // smoothed patch
    static constexpr int kNW = kTileW + 2 * RN, kNH = kTileH + 2 * RN;          // normals / Sobel cotangents
    static constexpr int kDW = kTileW + 2 * kB, kDH = kTileH + 2 * kB;          // cotangent of S
    static constexpr int kEIters = (kEW * kEH + kThreads - 1) / kThreads;
    static constexpr int kNIters = (kNW * kNH + kThreads - 1) / kThreads;
    static constexpr int kTileIters = kTileW * kTileH / kThreads;
    static_assert(kTileW * kTileH % kThreads == 0, "tile / workgroup shape");
};

struct Params {
    float w[5];                               // blur weights (SMOOTH only)
    float min_depth, max_depth, alpha_floor;
    double wsum2;                             // (sum of the five rounded weights)^2: what the blur makes of a constant 1
};

struct Row {                                  // one workgroup's partial sums: finalize_rows_kernel reads them as double[2]
    double sum, cnt;
};

__device__ __forceinline__ float nanf32() { return __builtin_nanf(""); }

// expected depth of a pixel, NaN when invalid; `thresholds`: min_depth / max_depth apply too (the normal-map form)
__device__ __forceinline__ float checked_depth(float d, float al, bool has_alpha, bool thresholds, const Params& P)
{
    const float E = expected_depth<float>(d, al, has_alpha, P.alpha_floor);
    bool ok = fabsf(E) < INFINITY && E > 0.0f;                                  // (NaN fails every comparison)
    if (thresholds) ok = ok && E > P.min_depth && E < P.max_depth;
    return ok ? E : nanf32();
}

__device__ __forceinline__ float target_depth(float g, const Params& P)
{
    return valid_depth(g, P.min_depth, P.max_depth) ? g : nanf32();
}

// v[k]: the depth (NaN = invalid) of patch element t + k * kThreads at its clamped coordinate.  Leaves the smoothed patch in
// s_s (every position: the value of its clamped coordinate) and ends with a barrier; s_e and s_h are free afterwards.
//
// The patch is kept RELATIVE to one depth of its own, c = the smallest valid depth of the patch (an exact, order-independent
// reduction): s_s holds S - c_eff and c_eff is returned.  The normals need differences of S between neighbours, a few
// thousandths of S at a realistic focal length; carried as S itself in fp32 those differences lose three digits to
// cancellation, carried relative to c they do not (E - c is exact for E < 2 c).  The blur of a constant c is c * wsum2, so
// c_eff = c * wsum2 (c itself without smoothing); sobel_points() adds the constant's own contribution back in closed form.
template <bool SMOOTH, int RN>
__device__ __forceinline__ float build_map(const float (&v)[Geo<SMOOTH, RN>::kEIters], const Params& P, int x0, int y0, int H, int W,
                                           float* __restrict__ s_e, float* __restrict__ s_h, float* __restrict__ s_s,
                                           unsigned* __restrict__ s_min)
{
    using G = Geo<SMOOTH, RN>;
    const int t = threadIdx.x;
    if (t == 0) *s_min = 0x7f800000u;                                           // +inf
    __syncthreads();
    float m = INFINITY;
#pragma unroll
    for (int k = 0; k < G::kEIters; ++k)
        if (t + k * kThreads < G::kEW * G::kEH && v[k] > 0.0f) m = fminf(m, v[k]);   // (positive floats order as their bits)
    if (m < INFINITY) atomicMin(s_min, __float_as_uint(m));
    __syncthreads();
    const float lowest = __uint_as_float(*s_min);
    const float c = lowest < INFINITY ? lowest : 0.0f;
    float* dst = SMOOTH ? s_e : s_s;                                            // (without smoothing the two patches coincide)
#pragma unroll
    for (int k = 0; k < G::kEIters; ++k) {
        const int i = t + k * kThreads;
        if (i < G::kEW * G::kEH) dst[i] = v[k] - c;
    }
    __syncthreads();
    if constexpr (SMOOTH) {
        // rows: every row of the depth patch; columns: those of the smoothed patch, the window centred on the clamped column
        for (int i = t; i < G::kEH * G::kSW; i += kThreads) {
            const int ly = i / G::kSW, lx = i - ly * G::kSW;
            const int xc = min(max(x0 - G::kHS + lx, 0), W - 1);
            const float* e = s_e + ly * G::kEW + (xc - (x0 - G::kHE));
            s_h[i] = (((P.w[0] * e[-2] + P.w[1] * e[-1]) + P.w[2] * e[0]) + P.w[3] * e[1]) + P.w[4] * e[2];
        }
        __syncthreads();
        for (int i = t; i < G::kSH * G::kSW; i += kThreads) {
            const int ly = i / G::kSW, lx = i - ly * G::kSW;
            const int yc = min(max(y0 - G::kHS + ly, 0), H - 1);
            const float* h = s_h + (yc - (y0 - G::kHE)) * G::kSW + lx;
            s_s[i] = (((P.w[0] * h[-2 * G::kSW] + P.w[1] * h[-G::kSW]) + P.w[2] * h[0]) + P.w[3] * h[G::kSW]) + P.w[4] * h[2 * G::kSW];
        }
        __syncthreads();
        return (float)((double)c * P.wsum2);
    }
    return c;
}

struct Rays {                                  // (px - cx) / fx of the three tap columns, (py - cy) / fy of the three tap rows,
    float x[3], y[3];                          // and the ray differences between the outer taps (from the integer distance:
    float dx, dy;                              // x[2] - x[0] would cancel)
};

__device__ __forceinline__ Rays rays_at(int y, int x, int H, int W, float fx, float fy, float cx, float cy)
{
    Rays r;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.x[k] = ((float)min(max(x + k - 1, 0), W - 1) - cx) / fx;
        r.y[k] = ((float)min(max(y + k - 1, 0), H - 1) - cy) / fy;
    }
    r.dx = (float)(min(x + 1, W - 1) - max(x - 1, 0)) / fx;
    r.dy = (float)(min(y + 1, H - 1) - max(y - 1, 0)) / fy;
    return r;
}

// The Sobel vectors (/ 8) of the camera-space points of the 3 x 3 depth patch whose top-left element is p[0], rows `stride`
// apart; the patch holds S - c.  The constant c leaves four of the six sums (its taps cancel) and adds c / 2 times the ray
// difference of the outer taps to Gx.x and Gy.y.  false: one of the nine taps is invalid.
__device__ __forceinline__ bool sobel_points(const float* p, int stride, const Rays& r, float c, float (&Gx)[3], float (&Gy)[3])
{
    const float a00 = p[0], a01 = p[1], a02 = p[2];
    const float a10 = p[stride], a11 = p[stride + 1], a12 = p[stride + 2];
    const float a20 = p[2 * stride], a21 = p[2 * stride + 1], a22 = p[2 * stride + 2];
    const float all = (((a00 + a01) + (a02 + a10)) + ((a11 + a12) + (a20 + a21))) + a22;   // NaN iff a tap is NaN (the others are finite)
    const float x0 = r.x[0], x1 = r.x[1], x2 = r.x[2], y0 = r.y[0], y1 = r.y[1], y2 = r.y[2];
    Gx[0] = 0.125f * (((a02 * x2 - a00 * x0) + (a22 * x2 - a20 * x0)) + 2.0f * (a12 * x2 - a10 * x0)) + c * (0.5f * r.dx);
    Gy[0] = 0.125f * (((a20 * x0 - a00 * x0) + (a22 * x2 - a02 * x2)) + 2.0f * (a21 * x1 - a01 * x1));
    Gx[1] = 0.125f * (((a02 * y0 - a00 * y0) + (a22 * y2 - a20 * y2)) + 2.0f * (a12 * y1 - a10 * y1));
    Gy[1] = 0.125f * (((a20 * y2 - a00 * y0) + (a22 * y2 - a02 * y0)) + 2.0f * (a21 * y2 - a01 * y0)) + c * (0.5f * r.dy);
    Gx[2] = 0.125f * (((a02 - a00) + (a22 - a20)) + 2.0f * (a12 - a10));
    Gy[2] = 0.125f * (((a20 - a00) + (a22 - a02)) + 2.0f * (a21 - a01));
    return all == all;
}

__device__ __forceinline__ double dot3(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// From the two fp32 Sobel vectors on, a pixel is carried in fp64: 1 - n . t is a difference of two numbers near 1, and the
// normalise Jacobian's c - n (n . c) one of two nearly equal vectors; rounded to fp32, n alone would put 6e-8 on a term of 1e-2.
// The fp64 rate of the chip is half its fp32 rate, and these are some tens of operations per pixel.
__device__ __forceinline__ void cross3(const float (&a)[3], const float (&b)[3], double (&c)[3])
{
    const double a0 = a[0], a1 = a[1], a2 = a[2], b0 = b[0], b1 = b[1], b2 = b[2];
    c[0] = a1 * b2 - a2 * b1;
    c[1] = a2 * b0 - a0 * b2;
    c[2] = a0 * b1 - a1 * b0;
}

// raw = Gx x Gy of the patch at p and inv = 1 / max(|raw|, eps): n = raw * inv (one fp64 division per normal).  false: invalid
// (raw and inv are then not to be used)
__device__ __forceinline__ bool raw_normal_at(const float* p, int stride, const Rays& r, float c, double (&raw)[3], double& inv)
{
    float Gx[3], Gy[3];
    const bool ok = sobel_points(p, stride, r, c, Gx, Gy);
    cross3(Gx, Gy, raw);
    inv = 1.0 / fmax(sqrt(dot3(raw, raw)), (double)kNormEps);
    return ok;
}

__device__ __forceinline__ bool normal_at(const float* p, int stride, const Rays& r, float c, double (&n)[3])
{
    double inv;
    const bool ok = raw_normal_at(p, stride, r, c, n, inv);
#pragma unroll
    for (int k = 0; k < 3; ++k) n[k] *= inv;
    return ok;
}

__device__ __forceinline__ bool finite3(const float (&v)[3])
{
    return fabsf(v[0]) < INFINITY && fabsf(v[1]) < INFINITY && fabsf(v[2]) < INFINITY;
}

// One tile of one view.  blockIdx.x = view * tiles + tile.  MODE kGtDepth / kGtNormals: rows[blockIdx.x] receives the partial
// sums; kMap: normals [B,3,H,W] receives the tile's normals.
template <bool SMOOTH, int MODE>
__global__ __launch_bounds__(kThreads) void normals_fwd_kernel(int H, int W, int tiles_x, int tiles, const float* __restrict__ depth,
                                                               const float* __restrict__ alpha, const float* __restrict__ intr,
                                                               const float* __restrict__ gt_depth,
                                                               const float* __restrict__ gt_normals, Params P,
                                                               float* __restrict__ normals, Row* __restrict__ rows)
{
    using G = Geo<SMOOTH, 0>;
    __shared__ float s_e[SMOOTH ? G::kEH * G::kEW : 1], s_h[SMOOTH ? G::kEH * G::kSW : 1];
    __shared__ float s_s[G::kSH * G::kSW], s_t[MODE == kGtDepth ? G::kSH * G::kSW : 1];
    __shared__ double s_red[MODE == kMap ? 1 : 2 * kThreads];
    __shared__ unsigned s_min;
    const int t = threadIdx.x;
    const long long view = blockIdx.x / tiles;
    const int tile = blockIdx.x - (int)(view * tiles);
    const int x0 = (tile % tiles_x) * kTileW, y0 = (tile / tiles_x) * kTileH;
    const size_t plane = (size_t)H * W, base = (size_t)view * plane;
    const float fx = intr[view * 4], fy = intr[view * 4 + 1], cx = intr[view * 4 + 2], cy = intr[view * 4 + 3];

    // every load of the thread is issued before the first value is used; a slot past the patch reads a clamped, in-range
    // address and is dropped
    float v_d[G::kEIters], v_a[G::kEIters], v_g[G::kEIters], v_t[G::kTileIters][3];
#pragma unroll
    for (int k = 0; k < G::kEIters; ++k) {
        const int i = t + k * kThreads;
        const int ly = i / G::kEW, lx = i - ly * G::kEW;
        const int yc = min(max(y0 - G::kHE + ly, 0), H - 1), xc = min(max(x0 - G::kHE + lx, 0), W - 1);
        const size_t o = base + (size_t)yc * W + xc;
        v_d[k] = depth[o];
        v_a[k] = alpha ? alpha[o] : 1.0f;
        v_g[k] = MODE == kGtDepth ? gt_depth[o] : 0.0f;
    }
    if constexpr (MODE == kGtNormals) {
#pragma unroll
        for (int k = 0; k < G::kTileIters; ++k) {
            const int i = t + k * kThreads;
            const int yc = min(y0 + i / kTileW, H - 1), xc = min(x0 + i % kTileW, W - 1);
#pragma unroll
            for (int c = 0; c < 3; ++c) v_t[k][c] = gt_normals[(size_t)view * 3 * plane + c * plane + (size_t)yc * W + xc];
        }
    }
#pragma unroll
    for (int k = 0; k < G::kEIters; ++k) {
        v_d[k] = checked_depth(v_d[k], v_a[k], alpha != nullptr, MODE == kMap, P);
        v_g[k] = target_depth(v_g[k], P);
    }
    const float c_s = build_map<SMOOTH, 0>(v_d, P, x0, y0, H, W, s_e, s_h, s_s, &s_min);
    float c_t = 0.0f;
    if constexpr (MODE == kGtDepth) c_t = build_map<SMOOTH, 0>(v_g, P, x0, y0, H, W, s_e, s_h, s_t, &s_min);

    double sum = 0.0;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < G::kTileIters; ++k) {
        const int i = t + k * kThreads;
        const int ly = i / kTileW, lx = i - ly * kTileW;
        const int y = y0 + ly, x = x0 + lx;
        if (y >= H || x >= W) continue;
        const Rays r = rays_at(y, x, H, W, fx, fy, cx, cy);
        double n[3], tg[3], n_inv, t_inv = 1.0;                  // n and t unnormalised: n . t = (n . tg) n_inv t_inv
        const bool n_ok = raw_normal_at(&s_s[ly * G::kSW + lx], G::kSW, r, c_s, n, n_inv);
        if constexpr (MODE == kMap) {
#pragma unroll
            for (int c = 0; c < 3; ++c) normals[(size_t)view * 3 * plane + c * plane + (size_t)y * W + x] = n_ok ? (float)(n[c] * n_inv) : nanf32();
        } else {
            bool t_ok;
            if constexpr (MODE == kGtDepth) {
                t_ok = raw_normal_at(&s_t[ly * G::kSW + lx], G::kSW, r, c_t, tg, t_inv);
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) tg[c] = (double)v_t[k][c];
                t_ok = finite3(v_t[k]);
            }
            if (n_ok && t_ok) {
                sum += 0.5 * (1.0 - dot3(n, tg) * (n_inv * t_inv));
                ++cnt;
            }
        }
    }
    if constexpr (MODE != kMap) {
        double v[2] = {sum, (double)cnt};
        block_sum_tree<2>(v, s_red);
        if (t == 0) rows[blockIdx.x] = Row{v[0], v[1]};
    }
}

// 1-D weight of the blur output s = p + d on element p of an axis of n elements: the taps of s that land on p, the clamped ones
// included; 0 for an output outside the axis
__device__ __forceinline__ float blur_weight_on(int p, int d, int n, const Params& P)
{
    const int s = p + d;
    float w = 0.0f;
    if (s >= 0 && s < n) {
#pragma unroll
        for (int b = -2; b <= 2; ++b)
            if (min(max(s + b, 0), n - 1) == p) w += P.w[b + 2];
    }
    return w;
}

// One tile of one view, backward.  MODE kGtDepth / kGtNormals: g_sum [B] is the cotangent of the view's sum; kMap: g_normals
// [B,3,H,W] is the cotangent of the normal map.
template <bool SMOOTH, int MODE>
__global__ __launch_bounds__(kThreads) void normals_bwd_kernel(int H, int W, int tiles_x, int tiles, const float* __restrict__ depth,
                                                               const float* __restrict__ alpha, const float* __restrict__ intr,
                                                               const float* __restrict__ gt_depth,
                                                               const float* __restrict__ gt_normals, Params P,
                                                               const float* __restrict__ g_sum, const float* __restrict__ g_normals,
                                                               float* __restrict__ g_depth, float* __restrict__ g_alpha)
{
    constexpr int RN = SMOOTH ? 3 : 1;
    using G = Geo<SMOOTH, RN>;
    constexpr int kN = G::kNH * G::kNW;
    static_assert(G::kDH * G::kDW <= G::kEH * G::kEW, "the cotangent of S reuses the depth patch");
    __shared__ float s_e[SMOOTH ? G::kEH * G::kEW : 1], s_h[SMOOTH ? G::kEH * G::kSW : 1];
    __shared__ float s_s[G::kSH * G::kSW], s_t[MODE == kGtDepth ? G::kSH * G::kSW : 1];
    __shared__ float s_dg[6 * kN];                               // [component of (dGx, dGy)][pixel of the halo-RN region]
    __shared__ unsigned s_min;
    const int t = threadIdx.x;
    const long long view = blockIdx.x / tiles;
    const int tile = blockIdx.x - (int)(view * tiles);
    const int x0 = (tile % tiles_x) * kTileW, y0 = (tile / tiles_x) * kTileH;
    const size_t plane = (size_t)H * W, base = (size_t)view * plane;
    const float fx = intr[view * 4], fy = intr[view * 4 + 1], cx = intr[view * 4 + 2], cy = intr[view * 4 + 3];
    const float coef = MODE == kMap ? 0.0f : -0.5f * g_sum[view];

    // all loads first: the depth patch, the target (or the cotangent) on the halo-RN region, the thread's own pixels
    float v_d[G::kEIters], v_a[G::kEIters], v_g[G::kEIters], v_c[G::kNIters][3], own_d[G::kTileIters], own_a[G::kTileIters];
#pragma unroll
    for (int k = 0; k < G::kEIters; ++k) {
        const int i = t + k * kThreads;
        const int ly = i / G::kEW, lx = i - ly * G::kEW;
        const int yc = min(max(y0 - G::kHE + ly, 0), H - 1), xc = min(max(x0 - G::kHE + lx, 0), W - 1);
        const size_t o = base + (size_t)yc * W + xc;
        v_d[k] = depth[o];
        v_a[k] = alpha ? alpha[o] : 1.0f;
        v_g[k] = MODE == kGtDepth ? gt_depth[o] : 0.0f;
    }
    if constexpr (MODE != kGtDepth) {
        const float* src = (MODE == kGtNormals ? gt_normals : g_normals) + (size_t)view * 3 * plane;
#pragma unroll
        for (int k = 0; k < G::kNIters; ++k) {
            const int i = t + k * kThreads;
            const int ly = i / G::kNW, lx = i - ly * G::kNW;
            const int yc = min(max(y0 - RN + ly, 0), H - 1), xc = min(max(x0 - RN + lx, 0), W - 1);
#pragma unroll
            for (int c = 0; c < 3; ++c) v_c[k][c] = src[c * plane + (size_t)yc * W + xc];
        }
    }
#pragma unroll
    for (int k = 0; k < G::kTileIters; ++k) {
        const int i = t + k * kThreads;
        const int yc = min(y0 + i / kTileW, H - 1), xc = min(x0 + i % kTileW, W - 1);
        own_d[k] = depth[base + (size_t)yc * W + xc];
        own_a[k] = alpha ? alpha[base + (size_t)yc * W + xc] : 1.0f;
    }
#pragma unroll
    for (int k = 0; k < G::kEIters; ++k) {
        v_d[k] = checked_depth(v_d[k], v_a[k], alpha != nullptr, MODE == kMap, P);
        v_g[k] = target_depth(v_g[k], P);
    }
    const float c_s = build_map<SMOOTH, RN>(v_d, P, x0, y0, H, W, s_e, s_h, s_s, &s_min);
    float c_t = 0.0f;
    if constexpr (MODE == kGtDepth) c_t = build_map<SMOOTH, RN>(v_g, P, x0, y0, H, W, s_e, s_h, s_t, &s_min);

    // cotangents of the Sobel vectors of output q = (y0 - RN + ly, x0 - RN + lx), the 1 / 8 of the Sobel included; 0 outside the
    // image and where the output is not consumed
#pragma unroll
    for (int k = 0; k < G::kNIters; ++k) {
        const int i = t + k * kThreads;
        if (i >= kN) continue;
        const int ly = i / G::kNW, lx = i - ly * G::kNW;
        const int y = y0 - RN + ly, x = x0 - RN + lx;
        float dGx[3] = {0.0f, 0.0f, 0.0f}, dGy[3] = {0.0f, 0.0f, 0.0f};
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const Rays r = rays_at(y, x, H, W, fx, fy, cx, cy);
            float Gx[3], Gy[3];
            double raw[3], c[3];
            bool ok = sobel_points(&s_s[ly * G::kSW + lx], G::kSW, r, c_s, Gx, Gy);
            if constexpr (MODE == kGtDepth) {
                double tg[3];
                ok = normal_at(&s_t[ly * G::kSW + lx], G::kSW, r, c_t, tg) && ok;
#pragma unroll
                for (int j = 0; j < 3; ++j) c[j] = (double)coef * tg[j];
            } else if constexpr (MODE == kGtNormals) {
                ok = ok && finite3(v_c[k]);
#pragma unroll
                for (int j = 0; j < 3; ++j) c[j] = (double)coef * (double)v_c[k][j];
            } else {
#pragma unroll
                for (int j = 0; j < 3; ++j) c[j] = (double)v_c[k][j];
            }
            if (ok) {
                cross3(Gx, Gy, raw);
                const double nr = sqrt(dot3(raw, raw));
                const double inv = 1.0 / fmax(nr, (double)kNormEps);
                double dr[3];
                if (nr >= (double)kNormEps) {                    // n = raw / |raw|: the tangential part of c, / |raw|
                    const double n[3] = {raw[0] * inv, raw[1] * inv, raw[2] * inv};
                    const double nc = dot3(n, c);
#pragma unroll
                    for (int j = 0; j < 3; ++j) dr[j] = (c[j] - n[j] * nc) * inv;
                } else {                                         // beneath the floor the map is linear
#pragma unroll
                    for (int j = 0; j < 3; ++j) dr[j] = c[j] * inv;
                }
                const double gx[3] = {Gx[0], Gx[1], Gx[2]}, gy[3] = {Gy[0], Gy[1], Gy[2]};
                dGx[0] = (float)(0.125 * (gy[1] * dr[2] - gy[2] * dr[1]));       // Gy x dr
                dGx[1] = (float)(0.125 * (gy[2] * dr[0] - gy[0] * dr[2]));
                dGx[2] = (float)(0.125 * (gy[0] * dr[1] - gy[1] * dr[0]));
                dGy[0] = (float)(0.125 * (dr[1] * gx[2] - dr[2] * gx[1]));       // dr x Gx
                dGy[1] = (float)(0.125 * (dr[2] * gx[0] - dr[0] * gx[2]));
                dGy[2] = (float)(0.125 * (dr[0] * gx[1] - dr[1] * gx[0]));
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            s_dg[j * kN + i] = dGx[j];
            s_dg[(3 + j) * kN + i] = dGy[j];
        }
    }
    __syncthreads();

    // cotangent of S at p from the (at most nine) Sobel outputs p - 1, p, p + 1 per axis that read it, dotted with p's own ray.
    // 1-D weights: the smoothing taps (1, 2, 1) and the difference taps (-1, 0, 1) that land on p, the clamped ones of the
    // border outputs included.  (ny, nx): p in the halo-RN region's coordinates.
    auto cot_S = [&](int y, int x, int ny, int nx) -> float {
        const float lo_y = y == 0 ? 1.0f : 0.0f, hi_y = y == H - 1 ? 1.0f : 0.0f;
        const float lo_x = x == 0 ? 1.0f : 0.0f, hi_x = x == W - 1 ? 1.0f : 0.0f;
        const float wsy[3] = {1.0f, 2.0f + lo_y + hi_y, 1.0f}, wdy[3] = {1.0f, hi_y - lo_y, -1.0f};
        const float wsx[3] = {1.0f, 2.0f + lo_x + hi_x, 1.0f}, wdx[3] = {1.0f, hi_x - lo_x, -1.0f};
        float acc[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const int q = (ny - 1 + a) * G::kNW + (nx - 1 + b);
                const float wx = wsy[a] * wdx[b], wy = wdy[a] * wsx[b];          // (small integers: exact)
#pragma unroll
                for (int j = 0; j < 3; ++j) acc[j] += wx * s_dg[j * kN + q] + wy * s_dg[(3 + j) * kN + q];
            }
        const float rx = ((float)x - cx) / fx, ry = ((float)y - cy) / fy;
        return (rx * acc[0] + ry * acc[1]) + acc[2];
    };

    float* s_ds = s_e;                                           // (the depth patch is no longer read)
    if constexpr (SMOOTH) {
        for (int i = t; i < G::kDH * G::kDW; i += kThreads) {
            const int ly = i / G::kDW, lx = i - ly * G::kDW;
            const int y = y0 - G::kB + ly, x = x0 - G::kB + lx;
            s_ds[i] = (y >= 0 && y < H && x >= 0 && x < W) ? cot_S(y, x, ly + RN - G::kB, lx + RN - G::kB) : 0.0f;
        }
        __syncthreads();
    }

#pragma unroll
    for (int k = 0; k < G::kTileIters; ++k) {
        const int i = t + k * kThreads;
        const int ly = i / kTileW, lx = i - ly * kTileW;
        const int y = y0 + ly, x = x0 + lx;
        if (y >= H || x >= W) continue;
        float dE;
        if constexpr (SMOOTH) {
            // the (at most 25) blur outputs that read this pixel; an output outside the image has weight 0 and cotangent 0
            float wy[5], wx[5];
#pragma unroll
            for (int d = 0; d < 5; ++d) {
                wy[d] = blur_weight_on(y, d - 2, H, P);
                wx[d] = blur_weight_on(x, d - 2, W, P);
            }
            dE = 0.0f;
#pragma unroll
            for (int a = 0; a < 5; ++a) {
                float row = 0.0f;
#pragma unroll
                for (int b = 0; b < 5; ++b) row += wx[b] * s_ds[(ly + a) * G::kDW + lx + b];
                dE += wy[a] * row;
            }
        } else {
            dE = cot_S(y, x, ly + RN, lx + RN);
        }
        const float al = own_a[k];
        const float E = checked_depth(own_d[k], al, alpha != nullptr, MODE == kMap, P);
        float gd = 0.0f, ga = 0.0f;
        if (E == E) {                                            // an invalid pixel receives exactly 0
            if (alpha) {
                gd = dE / fmaxf(al, P.alpha_floor);
                ga = al > P.alpha_floor ? -(gd * E) : 0.0f;      // -dE E / alpha, max(alpha, floor) = alpha here
            } else {
                gd = dE;
            }
        }
        const size_t o = base + (size_t)y * W + x;
        g_depth[o] = gd;
        if (alpha) g_alpha[o] = ga;
    }
}

struct Grid {
    int tiles_x, tiles;
};

bool make_grid(int32_t B, int32_t H, int32_t W, Grid& g)
{
    if (B <= 0 || H <= 0 || W <= 0) return false;
    if ((long long)H * W > 0x7fffffffLL) return false;
    g.tiles_x = (W + kTileW - 1) / kTileW;
    const long long tiles = (long long)g.tiles_x * ((H + kTileH - 1) / kTileH);
    if ((long long)B * tiles > 0x7fffffffLL) return false;
    g.tiles = (int)tiles;
    return true;
}

// sigma 0: no smoothing.  The weights are normalised in double and rounded once.
bool make_params(float sigma, float min_depth, float max_depth, float alpha_floor, Params& P)
{
    if (min_depth != min_depth || max_depth != max_depth) return false;
    if (!(alpha_floor > 0.0f && alpha_floor < INFINITY)) return false;
    if (!(sigma >= 0.0f && sigma < INFINITY)) return false;
    P.min_depth = min_depth;
    P.max_depth = max_depth;
    P.alpha_floor = alpha_floor;
    double w[5] = {0.0, 0.0, 1.0, 0.0, 0.0}, total = 0.0;
    if (sigma > 0.0f)
        for (int k = -2; k <= 2; ++k) w[k + 2] = exp(-(double)(k * k) / (2.0 * (double)sigma * (double)sigma));
    for (int k = 0; k < 5; ++k) total += w[k];
    double sum = 0.0;
    for (int k = 0; k < 5; ++k) {
        P.w[k] = (float)(w[k] / total);
        sum += (double)P.w[k];
    }
    P.wsum2 = sum * sum;
    return true;
}

size_t rows_bytes(int32_t B, const Grid& g) { return align_up((size_t)B * g.tiles * sizeof(Row), 256); }

template <int MODE>
void launch_fwd(bool smooth, dim3 grid, hipStream_t st, int H, int W, const Grid& g, const float* depth, const float* alpha,
                const float* intr, const float* gt_depth, const float* gt_normals, const Params& P, float* normals, Row* rows)
{
    if (smooth)
        hipLaunchKernelGGL((normals_fwd_kernel<true, MODE>), grid, dim3(kThreads), 0, st, H, W, g.tiles_x, g.tiles, depth, alpha, intr,
                           gt_depth, gt_normals, P, normals, rows);
    else
        hipLaunchKernelGGL((normals_fwd_kernel<false, MODE>), grid, dim3(kThreads), 0, st, H, W, g.tiles_x, g.tiles, depth, alpha, intr,
                           gt_depth, gt_normals, P, normals, rows);
}

template <int MODE>
void launch_bwd(bool smooth, dim3 grid, hipStream_t st, int H, int W, const Grid& g, const float* depth, const float* alpha,
                const float* intr, const float* gt_depth, const float* gt_normals, const Params& P, const float* g_sum,
                const float* g_normals, float* g_depth, float* g_alpha)
{
    if (smooth)
        hipLaunchKernelGGL((normals_bwd_kernel<true, MODE>), grid, dim3(kThreads), 0, st, H, W, g.tiles_x, g.tiles, depth, alpha, intr,
                           gt_depth, gt_normals, P, g_sum, g_normals, g_depth, g_alpha);
    else
        hipLaunchKernelGGL((normals_bwd_kernel<false, MODE>), grid, dim3(kThreads), 0, st, H, W, g.tiles_x, g.tiles, depth, alpha, intr,
                           gt_depth, gt_normals, P, g_sum, g_normals, g_depth, g_alpha);
}

}  // namespace

}  // namespace fs

using namespace fs;

FS_API int fs_normals_api_version(void) { return FS_NORMALS_API_VERSION; }

FS_API size_t fs_normals_scratch_bytes(int32_t B, int32_t H, int32_t W)
{
    Grid g;
    if (!make_grid(B, H, W, g)) return 0;
    return rows_bytes(B, g);
}

FS_API int fs_depth_normals_forward(int32_t B, int32_t H, int32_t W, const float* depth, const float* alpha, const float* intrinsics,
                                    float sigma, float min_depth, float max_depth, float alpha_floor, float* normals, void* stream_)
{
    Grid g;
    Params P;
    if (!make_grid(B, H, W, g) || !make_params(sigma, min_depth, max_depth, alpha_floor, P) || !depth || !intrinsics || !normals)
        return FS_ERR_INVALID_ARG;
    launch_fwd<kMap>(sigma > 0.0f, dim3((unsigned)(B * g.tiles)), (hipStream_t)stream_, H, W, g, depth, alpha, intrinsics, nullptr,
                     nullptr, P, normals, nullptr);
    FS_CHECK_LAUNCH("depth_normals_forward");
    return FS_OK;
}

FS_API int fs_depth_normals_backward(int32_t B, int32_t H, int32_t W, const float* depth, const float* alpha, const float* intrinsics,
                                     float sigma, float min_depth, float max_depth, float alpha_floor, const float* g_normals,
                                     float* g_depth, float* g_alpha, void* stream_)
{
    Grid g;
    Params P;
    if (!make_grid(B, H, W, g) || !make_params(sigma, min_depth, max_depth, alpha_floor, P) || !depth || !intrinsics || !g_normals ||
        !g_depth || (alpha && !g_alpha))
        return FS_ERR_INVALID_ARG;
    launch_bwd<kMap>(sigma > 0.0f, dim3((unsigned)(B * g.tiles)), (hipStream_t)stream_, H, W, g, depth, alpha, intrinsics, nullptr,
                     nullptr, P, nullptr, g_normals, g_depth, g_alpha);
    FS_CHECK_LAUNCH("depth_normals_backward");
    return FS_OK;
}

FS_API int fs_normals_loss_forward(int32_t B, int32_t H, int32_t W, const float* depth, const float* alpha, const float* intrinsics,
                                   const float* gt_depth, const float* gt_normals, float sigma, float min_depth, float max_depth,
                                   float alpha_floor, double* sum, double* cnt, void* scratch, void* stream_)
{
    Grid g;
    Params P;
    if (!make_grid(B, H, W, g) || !make_params(sigma, min_depth, max_depth, alpha_floor, P) || !depth || !intrinsics ||
        (gt_depth != nullptr) == (gt_normals != nullptr) || !sum || !cnt || !scratch)
        return FS_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream_;
    Row* rows = static_cast<Row*>(scratch);
    const dim3 grid((unsigned)(B * g.tiles));
    if (gt_depth)
        launch_fwd<kGtDepth>(sigma > 0.0f, grid, st, H, W, g, depth, alpha, intrinsics, gt_depth, nullptr, P, nullptr, rows);
    else
        launch_fwd<kGtNormals>(sigma > 0.0f, grid, st, H, W, g, depth, alpha, intrinsics, nullptr, gt_normals, P, nullptr, rows);
    hipLaunchKernelGGL((finalize_rows_kernel<2, BlockSum::kTree, false>), dim3((unsigned)B), dim3(kThreads), 0, st, g.tiles, 1,
                       reinterpret_cast<const double*>(rows), RowOuts<2>{{sum, cnt}, {}, 1});
    FS_CHECK_LAUNCH("normals_loss_forward");
    return FS_OK;
}

FS_API int fs_normals_loss_backward(int32_t B, int32_t H, int32_t W, const float* depth, const float* alpha, const float* intrinsics,
                                    const float* gt_depth, const float* gt_normals, float sigma, float min_depth, float max_depth,
                                    float alpha_floor, const float* g_sum, float* g_depth, float* g_alpha, void* stream_)
{
    Grid g;
    Params P;
    if (!make_grid(B, H, W, g) || !make_params(sigma, min_depth, max_depth, alpha_floor, P) || !depth || !intrinsics ||
        (gt_depth != nullptr) == (gt_normals != nullptr) || !g_sum || !g_depth || (alpha && !g_alpha))
        return FS_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream_;
    const dim3 grid((unsigned)(B * g.tiles));
    if (gt_depth)
        launch_bwd<kGtDepth>(sigma > 0.0f, grid, st, H, W, g, depth, alpha, intrinsics, gt_depth, nullptr, P, g_sum, nullptr, g_depth,
                             g_alpha);
    else
        launch_bwd<kGtNormals>(sigma > 0.0f, grid, st, H, W, g, depth, alpha, intrinsics, nullptr, gt_normals, P, g_sum, nullptr, g_depth,
                               g_alpha);
    FS_CHECK_LAUNCH("normals_loss_backward");
    return FS_OK;
}
