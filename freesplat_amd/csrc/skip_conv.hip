// skip_conv.hip -- the encoder's full-resolution skip branch fused into the latent pack (encoder_freesplat.py:124-128, :302-316):
//   lat[v, p, c] = head[v, 1 + c, p] + relu(bias[c] + sum_k W[c, k] patch[v, p, k]),   dens[v, p] = head[v, 0, p]
// with W the Conv2d(3, 64, 7, stride 1, padding 3) weights, k over the 3 x 7 x 7 taps (zero padding) -- the outputs and layouts
// of fs_latents_pack_forward, without the [V, 64, H, W] skip map ever existing in memory, forward or backward.
//
// Geometry (both directions): a workgroup of 4 wavefronts owns an 8 x 32 pixel tile at a time (and walks tiles
// blockIdx.x, blockIdx.x + gridDim.x, ...); the 3-channel image tile with its 3-pixel halo (3 x 14 x 38 floats, rows padded
// to 40) is staged in LDS.  A wavefront owns two image rows of 32 pixels.  All products run on v_mfma_f32_32x32x2_f32: fp32
// operands, fp32 accumulation -- no reduced-precision operand anywhere (the tests hold the result to the fp32 dot-product bound).
//
// Forward: D[channel][pixel] = W[channel][k] patch[k][pixel], K = 148 (147 taps + one zero column), the 64 x 148 weights
// k-major in LDS for the whole launch, the accumulators preloaded with the bias.  A lane of the result holds one pixel and 32 of
// its channels, which is the layout the channel-major head map is read in (128 B per channel and row segment); the sum goes
// through a per-wavefront LDS transpose so that every pixel's 64 channels leave as one 256-byte row (float4 per lane, 1 KB per
// store instruction).  The ReLU decision is kept as one bit per (pixel, channel): 8 bytes per pixel in `saved`.
//
// Backward: g_head is the transposed g_lat (channel 0 <- g_dens), written from the same LDS tile of g_lat the weight
// gradient reads.  g_weight[c][k] = sum_{v,p} mask g_lat[v, p, c] patch[v, p, k] is D[channel][tap] = G[channel][pixel]
// patch[pixel][tap], contracted over the pixels of the tile; tap 147 is a column of ones, so the bias gradient is row 147 of the
// same product.  Every wavefront accumulates its pixels over all the tiles of its workgroup in registers (2 x 5 blocks of
// 32 x 32); at the end the four wavefronts add up in LDS in the order 0, 1, 2, 3 and the workgroup writes ONE partial
// [64][160] to scratch; a second kernel adds the partials of an element in a fixed order (16 interleaved chains over the
// workgroups, then the 16 chains in order).
//
// Deterministic: no atomics of any kind.  The number of workgroups and the tile -> workgroup assignment depend on (V, H, W)
// only, every sum has a fixed order, so g_weight and g_bias have the same bits run to run and on any stream
// (tests/test_skip_latents_hip.py::test_backward_is_bit_reproducible).
#include "fs_common.h"

namespace fs {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kC = 64;                       // output channels
constexpr int kTaps = 147;                   // 3 x 7 x 7
constexpr int kK = 148;                      // taps padded to the MFMA's k step of 2
constexpr int kTW = 32, kTH = 8;             // pixel tile of a workgroup
constexpr int kHalo = 3;
constexpr int kTileW = kTW + 2 * kHalo, kTileH = kTH + 2 * kHalo;   // 38 x 14
constexpr int kRow = 40, kPlane = kTileH * kRow;                    // LDS row / channel-plane stride of the image tile
constexpr int kTileFloats = 3 * kPlane;
constexpr int kStage = kC + 4;               // row stride of the pixel-major staging tiles (float4-aligned)
constexpr int kThreads = 256;
constexpr int kMaxGroups = 512;              // workgroups of a launch: two per compute unit of an MI355X
constexpr int kTapCols = 160;                // taps padded to 5 MFMA blocks of 32 (backward)
constexpr int kPartial = kC * kTapCols;      // floats of one workgroup's weight-gradient partial
constexpr int kFinElems = 16, kFinChains = 16;

__host__ __device__ constexpr int tap_off(int k) { return (k / 49) * kPlane + ((k % 49) / 7) * kRow + k % 7; }
// row of a 32x32 MFMA result held in register r of a lane of half hh (column = lane & 31)
__device__ __forceinline__ constexpr int mfma_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

__device__ __forceinline__ f32x16 mfma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

struct Tile {
    int v, y0, x0;
};
__device__ __forceinline__ Tile tile_at(int t, int tx, int ty)
{
    Tile o;
    o.v = t / (tx * ty);
    const int r = t - o.v * (tx * ty);
    o.y0 = (r / tx) * kTH;
    o.x0 = (r % tx) * kTW;
    return o;
}

// the image tile with its halo, zero outside the image (the convolution's zero padding)
__device__ __forceinline__ void load_image_tile(const float* __restrict__ img, const Tile& tl, int h, int w, float* s_tile)
{
    for (int e = threadIdx.x; e < 3 * kTileH * kTileW; e += kThreads) {
        const int ci = e / (kTileH * kTileW), r = e - ci * (kTileH * kTileW), ry = r / kTileW, rx = r - ry * kTileW;
        const int gy = tl.y0 - kHalo + ry, gx = tl.x0 - kHalo + rx;
        float val = 0.0f;
        if (gy >= 0 && gy < h && gx >= 0 && gx < w) val = img[((size_t)(tl.v * 3 + ci) * h + gy) * w + gx];
        s_tile[ci * kPlane + ry * kRow + rx] = val;
    }
}

__global__ __launch_bounds__(kThreads, 2) void skip_latents_fwd_kernel(int h, int w, int tx, int ty, int n_tiles,
                                                                    const float* __restrict__ head,
                                                                    const float* __restrict__ img,
                                                                    const float* __restrict__ weight,
                                                                    const float* __restrict__ bias, float* __restrict__ lat,
                                                                    float* __restrict__ dens, uint2* __restrict__ saved)
{
    __shared__ float s_w[kK * kC];                                   // [k][channel]
    __shared__ float s_bias[kC];
    __shared__ float s_tile[kTileFloats];
    __shared__ __attribute__((aligned(16))) float s_stage[4][kTW * kStage];
    const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int i = lane & 31, hh = lane >> 5;
    const size_t P = (size_t)h * w;
    for (int e = t; e < kC * kTaps; e += kThreads) {
        const int c = e / kTaps, k = e - c * kTaps;
        s_w[k * kC + c] = weight[e];
    }
    if (t < kC) {
        s_w[kTaps * kC + t] = 0.0f;
        s_bias[t] = bias[t];
    }
    const float* wa = s_w + hh * kC + i;
    const float* tb = s_tile + 2 * wv * kRow + i;
    float* st = s_stage[wv];

    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const Tile tl = tile_at(tile, tx, ty);
        __syncthreads();                     // the previous tile's readers are done (first pass: nothing to wait for)
        load_image_tile(img, tl, h, w, s_tile);
        __syncthreads();                     // (first pass: also the weights)
        if (dens) {                          // the density logit: channel 0 of the head, one pixel per thread
            const int gy = tl.y0 + (t >> 5), gx = tl.x0 + (t & 31);
            if (gy < h && gx < w) {
                const size_t p = (size_t)gy * w + gx;
                dens[(size_t)tl.v * P + p] = head[(size_t)tl.v * (kC + 1) * P + p];
            }
        }
        f32x16 acc[2][2];                    // [channel block][row of the wavefront]
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float b = s_bias[32 * m + mfma_row(r, hh)];
                acc[m][0][r] = b;
                acc[m][1][r] = b;
            }
#pragma unroll
        for (int s = 0; s < kK / 2; ++s) {   // lane half hh takes tap 2 s + hh of the step
            const float a0 = wa[2 * s * kC], a1 = wa[2 * s * kC + 32];
            const int off = hh ? tap_off(2 * s + 1 < kTaps ? 2 * s + 1 : kTaps - 1) : tap_off(2 * s);
            float b0 = tb[off], b1 = tb[off + kRow];
            if (2 * s + 1 >= kTaps) {        // the padding column: weight 0 times 0
                b0 = hh ? 0.0f : b0;
                b1 = hh ? 0.0f : b1;
            }
            acc[0][0] = mfma(a0, b0, acc[0][0]);
            acc[1][0] = mfma(a1, b0, acc[1][0]);
            acc[0][1] = mfma(a0, b1, acc[0][1]);
            acc[1][1] = mfma(a1, b1, acc[1][1]);
        }
        // epilogue, one image row (32 pixels) at a time: ReLU + its bits, + head, transpose through LDS, 256-byte rows out
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int gy = tl.y0 + 2 * wv + n, gx = tl.x0 + i;
            const bool valid = gy < h && gx < w;
            const size_t p = valid ? (size_t)gy * w + gx : 0;
            const float* hp = head + ((size_t)tl.v * (kC + 1) + 1) * P + p;
            uint32_t bits[2] = {0u, 0u};
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float o[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int r = 4 * g + j, c = 32 * m + mfma_row(r, hh);
                        const float pre = acc[m][n][r];
                        const bool on = pre > 0.0f;
                        bits[m] |= on ? (1u << (c & 31)) : 0u;
                        const float hv = valid ? hp[(size_t)c * P] : 0.0f;
                        o[j] = hv + (on ? pre : 0.0f);
                    }
                    *(float4*)(st + i * kStage + 32 * m + 8 * g + 4 * hh) = make_float4(o[0], o[1], o[2], o[3]);
                }
            if (saved) {                     // the two lane halves hold disjoint channels of the same pixel
                bits[0] |= (uint32_t)__shfl_xor((int)bits[0], 32);
                bits[1] |= (uint32_t)__shfl_xor((int)bits[1], 32);
                if (valid && hh == 0) saved[(size_t)tl.v * P + p] = make_uint2(bits[0], bits[1]);
            }
            wave_lds_sync();
            if (gy < h) {
                float* orow = lat + ((size_t)tl.v * P + (size_t)gy * w + tl.x0) * kC;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int e = k * 64 + lane, q = e >> 4, c4 = (e & 15) * 4;
                    if (tl.x0 + q < w) *(float4*)(orow + (size_t)q * kC + c4) = *(const float4*)(st + q * kStage + c4);
                }
            }
            wave_lds_sync();
        }
    }
}

// partials == NULL: no weight / bias gradient wanted (only g_head); g_head == NULL: only the weight / bias gradient
__global__ __launch_bounds__(kThreads, 2) void skip_latents_bwd_kernel(int h, int w, int tx, int ty, int n_tiles,
                                                                    const float* __restrict__ img,
                                                                    const uint2* __restrict__ saved,
                                                                    const float* __restrict__ g_lat,
                                                                    const float* __restrict__ g_dens,
                                                                    float* __restrict__ g_head, float* __restrict__ partials)
{
    __shared__ float s_tile[kTileFloats];
    __shared__ __attribute__((aligned(16))) float s_stage[4][64 * kStage];   // g_lat of a wavefront's 64 pixels, pixel-major
    __shared__ uint2 s_mask[4][64];
    static_assert(4 * 64 * kStage >= kPartial, "the staging tiles double as the wavefront reduction buffer");
    const int t = threadIdx.x, lane = t & 63, wv = __builtin_amdgcn_readfirstlane(t >> 6);
    const int i = lane & 31, hh = lane >> 5;
    const size_t P = (size_t)h * w;
    float* st = s_stage[wv];
    int toff[5];
#pragma unroll
    for (int nb = 0; nb < 5; ++nb) {
        const int k = 32 * nb + i;
        toff[nb] = k < kTaps ? (k / 49) * kPlane + ((k % 49) / 7) * kRow + k % 7 : 0;
    }
    const bool ones = 128 + i == kTaps;      // this lane's column of block 4 is the bias column
    f32x16 acc[2][5];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nb = 0; nb < 5; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][nb][r] = 0.0f;

    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const Tile tl = tile_at(tile, tx, ty);
        __syncthreads();
        if (partials) load_image_tile(img, tl, h, w, s_tile);
#pragma unroll
        for (int n = 0; n < 2; ++n) {        // g_lat rows of 256 bytes in, zero outside the image
            const int gy = tl.y0 + 2 * wv + n;
            const float* grow = g_lat ? g_lat + ((size_t)tl.v * P + (size_t)(gy < h ? gy : 0) * w + tl.x0) * kC : nullptr;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int e = k * 64 + lane, q = e >> 4, c4 = (e & 15) * 4;
                float4 g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (grow && gy < h && tl.x0 + q < w) g = *(const float4*)(grow + (size_t)q * kC + c4);
                *(float4*)(st + (n * 32 + q) * kStage + c4) = g;
            }
        }
        const int gy = tl.y0 + 2 * wv + hh, gx = tl.x0 + i;       // this lane's pixel of the wavefront's 64
        const bool valid = gy < h && gx < w;
        const size_t p = valid ? (size_t)gy * w + gx : 0;
        s_mask[wv][lane] = partials && valid ? saved[(size_t)tl.v * P + p] : make_uint2(0u, 0u);
        __syncthreads();
        if (g_head && valid) {
            float* hp = g_head + (size_t)tl.v * (kC + 1) * P + p;
            hp[0] = g_dens ? g_dens[(size_t)tl.v * P + p] : 0.0f;
#pragma unroll 8
            // (row stride 68: 16 distinct banks over the 64 lanes, a 4-way conflict on 64 reads per tile -- small beside the
            //  640 MFMAs of the tile, and the stride keeps the float4 writes above aligned)
            for (int c = 0; c < kC; ++c) hp[(size_t)(1 + c) * P] = st[lane * kStage + c];
        }
        if (partials) {
#pragma unroll
            for (int s = 0; s < 32; ++s) {   // lane half hh takes pixel 2 s + hh of the wavefront's 64
                const int pix = 2 * s + hh;
                const uint2 mk = s_mask[wv][pix];
                float a0 = st[pix * kStage + i], a1 = st[pix * kStage + 32 + i];
                a0 = (mk.x >> i) & 1u ? a0 : 0.0f;
                a1 = (mk.y >> i) & 1u ? a1 : 0.0f;
                const float* tb = s_tile + (2 * wv + (s >> 4)) * kRow + ((2 * s) & 31) + hh;
#pragma unroll
                for (int nb = 0; nb < 5; ++nb) {
                    // block 4 holds taps 128 .. 159: 128 .. 146 are real, 147 is the column of ones, 148 .. 159 re-read tap 0
                    // (toff = 0) and accumulate values nobody reads -- the finishing kernel takes columns k < 148 only.  12 of
                    // 160 columns, 7.5 % of the MFMAs, are spent on them
                    float b = tb[toff[nb]];
                    if (nb == 4) b = ones ? 1.0f : b;
                    acc[0][nb] = mfma(a0, b, acc[0][nb]);
                    acc[1][nb] = mfma(a1, b, acc[1][nb]);
                }
            }
        }
    }
    if (!partials) return;
    // the four wavefronts in the order 0, 1, 2, 3, then one partial per workgroup
    float* red = &s_stage[0][0];
    for (int k = 0; k < 4; ++k) {
        __syncthreads();
        if (wv == k) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int nb = 0; nb < 5; ++nb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int idx = (32 * m + mfma_row(r, hh)) * kTapCols + 32 * nb + i;
                        red[idx] = k ? red[idx] + acc[m][nb][r] : acc[m][nb][r];
                    }
        }
    }
    __syncthreads();
    float* out = partials + (size_t)blockIdx.x * kPartial;
    for (int e = t; e < kPartial; e += kThreads) out[e] = red[e];
}

// g_weight [64][147] and g_bias [64] from the G partials [64][160]: a workgroup takes 16 consecutive elements of the
// [64][148] result; chain j of an element adds workgroups j, j + 16, ... in order, then the 16 chains are added in order
__global__ __launch_bounds__(kFinElems* kFinChains) void skip_wgrad_finish_kernel(int G, const float* __restrict__ partials,
                                                                                  float* __restrict__ g_weight,
                                                                                  float* __restrict__ g_bias)
{
    __shared__ float s_red[kFinChains][kFinElems];
    const int t = threadIdx.x, el = t % kFinElems, chain = t / kFinElems;
    const int e = blockIdx.x * kFinElems + el;      // < 64 * 148 (the grid covers it exactly)
    const int c = e / kK, k = e - c * kK;
    const float* src = partials + c * kTapCols + k;
    float v = 0.0f;
#pragma unroll 8
    for (int g = chain; g < G; g += kFinChains) v += src[(size_t)g * kPartial];
    s_red[chain][el] = v;
    __syncthreads();
    if (chain == 0) {
        v = 0.0f;
        for (int j = 0; j < kFinChains; ++j) v += s_red[j][el];
        if (k < kTaps) {
            if (g_weight) g_weight[c * kTaps + k] = v;
        } else if (g_bias) {
            g_bias[c] = v;
        }
    }
}
static_assert((kC * kK) % kFinElems == 0, "the finishing grid covers the [64][148] result exactly");

bool dims_ok(int32_t V, int32_t H, int32_t W)
{
    if (V <= 0 || H <= 0 || W <= 0) return false;
    const long long tiles = (long long)V * ((H + kTH - 1) / kTH) * ((W + kTW - 1) / kTW);
    return (long long)H * W <= 0x7fffffffLL && tiles <= 0x7fffffffLL;
}
int tiles_x(int32_t W) { return (W + kTW - 1) / kTW; }
int tiles_y(int32_t H) { return (H + kTH - 1) / kTH; }
int groups_for(int n_tiles) { return n_tiles < kMaxGroups ? n_tiles : kMaxGroups; }
bool shape_supported(int32_t c_in, int32_t c_out, int32_t ksize) { return c_in == 3 && c_out == kC && ksize == 7; }

}  // namespace

}  // namespace fs

using namespace fs;

FS_API size_t fs_skip_latents_saved_bytes(int32_t V, int32_t H, int32_t W)
{
    if (!dims_ok(V, H, W)) return 0;
    return (size_t)V * H * W * sizeof(uint2);
}

FS_API size_t fs_skip_latents_scratch_bytes(int32_t V, int32_t H, int32_t W)
{
    if (!dims_ok(V, H, W)) return 0;
    return (size_t)groups_for(V * tiles_x(W) * tiles_y(H)) * kPartial * sizeof(float);
}

FS_API int fs_skip_latents_forward(int32_t V, int32_t H, int32_t W, int32_t c_in, int32_t c_out, int32_t ksize,
                                   const float* head, const float* images, const float* weight, const float* bias,
                                   float* latents, float* dens, void* saved, void* stream_)
{
    if (V <= 0 || H <= 0 || W <= 0 || c_in <= 0 || c_out <= 0 || ksize <= 0 || !head || !images || !weight || !bias || !latents)
        return FS_ERR_INVALID_ARG;
    if (!shape_supported(c_in, c_out, ksize)) return FS_ERR_UNSUPPORTED;
    if (!dims_ok(V, H, W)) return FS_ERR_INVALID_ARG;
    ScopedStage prof_(kStEncoderTail, (hipStream_t)stream_);
    const int tx = tiles_x(W), ty = tiles_y(H), n_tiles = V * tx * ty;
    hipLaunchKernelGGL(skip_latents_fwd_kernel, dim3((unsigned)groups_for(n_tiles)), dim3(kThreads), 0, (hipStream_t)stream_, H, W,
                       tx, ty, n_tiles, head, images, weight, bias, latents, dens, static_cast<uint2*>(saved));
    FS_CHECK_LAUNCH("skip_latents_forward");
    return FS_OK;
}

FS_API int fs_skip_latents_backward(int32_t V, int32_t H, int32_t W, int32_t c_in, int32_t c_out, int32_t ksize,
                                    const float* images, const void* saved, const float* g_latents, const float* g_dens,
                                    float* g_head, float* g_weight, float* g_bias, void* scratch, void* stream_)
{
    const bool want_w = g_weight || g_bias;
    if (V <= 0 || H <= 0 || W <= 0 || c_in <= 0 || c_out <= 0 || ksize <= 0 || (!g_head && !want_w) ||
        (want_w && (!images || !saved || !scratch)))
        return FS_ERR_INVALID_ARG;
    if (!shape_supported(c_in, c_out, ksize)) return FS_ERR_UNSUPPORTED;
    if (!dims_ok(V, H, W)) return FS_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream_;
    ScopedStage prof_(kStEncoderTail, st);
    const int tx = tiles_x(W), ty = tiles_y(H), n_tiles = V * tx * ty, G = groups_for(n_tiles);
    float* partials = want_w ? static_cast<float*>(scratch) : nullptr;
    hipLaunchKernelGGL(skip_latents_bwd_kernel, dim3((unsigned)G), dim3(kThreads), 0, st, H, W, tx, ty, n_tiles, images,
                       static_cast<const uint2*>(saved), g_latents, g_dens, g_head, partials);
    if (want_w)
        hipLaunchKernelGGL(skip_wgrad_finish_kernel, dim3(kC * kK / kFinElems), dim3(kFinElems * kFinChains), 0, st, G, partials,
                           g_weight, g_bias);
    FS_CHECK_LAUNCH("skip_latents_backward");
    return FS_OK;
}
