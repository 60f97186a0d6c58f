// gaussian_transform.hip -- similarity transforms of Gaussian scenes (include/freesplat_amd_transform.h): the table of a
// transform (fs_transform_prepare), the rotation of the degree 1 - 3 spherical harmonics (fs_sh_rotate) and the transform of
// means, scales, rotations, covariances and harmonics with its backward (fs_gaussians_transform_forward / _backward).
//
// Everything but the table moves bytes: at degree 3 a Gaussian is 48 SH floats in and out against 249 multiply-adds, the
// geometry arrays 3 to 9 floats against a 3 x 3 product.  A thread owns a run of consecutive Gaussians whose floats are a
// multiple of four in every array -- four Gaussians in means, scales, rotations and covariances, one (M = 16) or four in the
// harmonics -- so a run starts at a multiple of 16 bytes from its array's base: an array whose base is 16-byte aligned goes
// through float4 accesses, any other array and the last, partial run through dword accesses with a bound check.  A thread reads
// its whole run into registers before it writes any of it and no other thread touches the run, so every array may be
// transformed in place; the arithmetic of an element is the same explicit fmaf chain on either path, so the bits do not depend
// on the alignment or on the in-place choice.
//
// The table row of a Gaussian comes from its id.  Rows are 100 floats; when every lane of a wavefront names the same row (no
// ids at all, or the consecutive Gaussians of one view) the row's address is wave-uniform and its entries are read with scalar
// loads, otherwise each lane reads its own row through the vector cache.  Both paths run the same chains.  An id outside [0, V)
// forms no address and leaves the registers as loaded: the Gaussian is stored back bit for bit.
//
// The forward and the backward are one kernel: the backward loads R transposed, the conjugate quaternion and D transposed from
// the table (an address choice, not a register shuffle) and drops the translation.  No atomics, no scratch, no LDS.
#include "fs_reduce.h"

#include "../../include/freesplat_amd_transform.h"

namespace fs {

namespace {

constexpr int kThreads = 256;
constexpr int kRow = FS_TRANSFORM_TABLE_FLOATS;
constexpr int kGeomGroup = 4;                        // Gaussians of a thread in the geometry arrays
constexpr int kFlagMask = FS_TRANSFORM_SH_CHANNEL_MAJOR | FS_TRANSFORM_SH_TRANSPOSE | FS_TRANSFORM_QUAT_XYZW | FS_TRANSFORM_COV_FULL;

template <int S>
__device__ __forceinline__ void store_run(float* base, size_t off, size_t total, bool aligned, const float (&r)[S])
{
    if (aligned && off + S <= total) {
#pragma unroll
        for (int k = 0; k < S / 4; ++k)
            *reinterpret_cast<float4*>(base + off + 4 * k) = make_float4(r[4 * k], r[4 * k + 1], r[4 * k + 2], r[4 * k + 3]);
    } else {
#pragma unroll
        for (int k = 0; k < S; ++k)
            if (off + k < total) base[off + k] = r[k];
    }
}

// the table row of Gaussian n as an index, -1 for "pass through" (n beyond N, or an id outside [0, V))
__device__ __forceinline__ int row_of_gaussian(long long n, int N, int V, const long long* __restrict__ ids)
{
    if (n >= N) return -1;
    const long long id = ids ? ids[n] : 0;
    return id >= 0 && id < (long long)V ? (int)id : -1;
}

// f(row pointer) for the lanes that have a row; the pointer is wave-uniform (scalar loads) when all lanes agree on the row
template <class F>
__device__ __forceinline__ void with_row(int vid, const float* __restrict__ table, F&& f)
{
    const int v0 = __builtin_amdgcn_readfirstlane(vid);
    if (__all(vid == v0)) {
        if (v0 >= 0) f(table + (size_t)v0 * kRow);
    } else if (vid >= 0) {
        f(table + (size_t)vid * kRow);
    }
}

// ---- spherical harmonics -----------------------------------------------------------------------------------------------------

// c: the 3 M coefficients of one Gaussian, [M][3] or (CM) [3][M].  Bands 1 .. deg in place; band 0 is left as loaded.
template <int M, bool CM>
__device__ __forceinline__ void rotate_bands(float* c, const float* __restrict__ T, bool tr)
{
    constexpr int DEG = M == 16 ? 3 : M == 9 ? 2 : M == 4 ? 1 : 0;
    constexpr int kOff[3] = {FS_TRANSFORM_D1, FS_TRANSFORM_D2, FS_TRANSFORM_D3};
#pragma unroll
    for (int l = 1; l <= DEG; ++l) {
        const int n = 2 * l + 1, first = l * l;
        const float* __restrict__ D = T + kOff[l - 1];
        float x[3][7], acc[3];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
#pragma unroll
            for (int j = 0; j < n; ++j) x[ch][j] = c[CM ? ch * M + first + j : (first + j) * 3 + ch];
#pragma unroll
        for (int i = 0; i < n; ++i) {
#pragma unroll
            for (int j = 0; j < n; ++j) {
                const float d = D[tr ? j * n + i : i * n + j];
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) acc[ch] = j == 0 ? d * x[ch][0] : fmaf(d, x[ch][j], acc[ch]);
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[CM ? ch * M + first + i : (first + i) * 3 + ch] = acc[ch];
        }
    }
}

template <int M>
struct ShRun {
    static constexpr int G = M == 16 ? 1 : 4;        // Gaussians of a thread: 48, 108, 48, 12 floats for M = 16, 9, 4, 1
    static constexpr int S = G * 3 * M;
};

template <int M, bool CM>
__global__ __launch_bounds__(kThreads) void sh_rotate_kernel(int N, int V, int tr, const float* in, const float* __restrict__ table,
                                                             const long long* __restrict__ ids, float* out)
{
    constexpr int G = ShRun<M>::G, S = ShRun<M>::S;
    const long long n0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * G;
    if (n0 >= N) return;
    const size_t total = (size_t)N * 3 * M, off = (size_t)n0 * 3 * M;
    float v[S];
    load_run<S>(in, off, total, aligned16(in), v);
#pragma unroll
    for (int j = 0; j < G; ++j)
        with_row(row_of_gaussian(n0 + j, N, V, ids), table, [&](const float* __restrict__ T) { rotate_bands<M, CM>(v + j * 3 * M, T, tr != 0); });
    store_run<S>(out, off, total, aligned16(out), v);
}

// ---- geometry ----------------------------------------------------------------------------------------------------------------

// (s, E, t, p) of a row: E = R and p = q forward, E = R^T and p = conj(q) backward
struct Xf {
    float s, E[9], t[3], p[4];
};

__device__ __forceinline__ Xf load_xf(const float* __restrict__ T, bool bwd)
{
    Xf x;
    x.s = T[FS_TRANSFORM_S];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) x.E[i * 3 + j] = T[FS_TRANSFORM_R + (bwd ? j * 3 + i : i * 3 + j)];
#pragma unroll
    for (int i = 0; i < 3; ++i) x.t[i] = T[FS_TRANSFORM_T + i];
    x.p[0] = T[FS_TRANSFORM_Q];
#pragma unroll
    for (int i = 1; i < 4; ++i) x.p[i] = bwd ? -T[FS_TRANSFORM_Q + i] : T[FS_TRANSFORM_Q + i];
    return x;
}

__device__ __forceinline__ void xf_mean(float* m, const float* __restrict__ T, bool bwd)
{
    const Xf x = load_xf(T, bwd);
    float r[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i] = fmaf(x.E[i * 3 + 2], m[2], fmaf(x.E[i * 3 + 1], m[1], x.E[i * 3] * m[0]));
#pragma unroll
    for (int i = 0; i < 3; ++i) m[i] = bwd ? x.s * r[i] : fmaf(x.s, r[i], x.t[i]);
}

__device__ __forceinline__ void xf_scale(float* sc, const float* __restrict__ T)
{
    const float s = T[FS_TRANSFORM_S];
#pragma unroll
    for (int i = 0; i < 3; ++i) sc[i] = s * sc[i];
}

// q: (w, x, y, z), or (x, y, z, w) with xyzw
__device__ __forceinline__ void xf_quat(float* q, const float* __restrict__ T, bool bwd, bool xyzw)
{
    const Xf x = load_xf(T, bwd);
    const float gw = xyzw ? q[3] : q[0], gx = xyzw ? q[0] : q[1], gy = xyzw ? q[1] : q[2], gz = xyzw ? q[2] : q[3];
    const float pw = x.p[0], px = x.p[1], py = x.p[2], pz = x.p[3];
    const float ow = fmaf(-pz, gz, fmaf(-py, gy, fmaf(-px, gx, pw * gw)));
    const float ox = fmaf(-pz, gy, fmaf(py, gz, fmaf(px, gw, pw * gx)));
    const float oy = fmaf(pz, gx, fmaf(py, gw, fmaf(-px, gz, pw * gy)));
    const float oz = fmaf(pz, gw, fmaf(-py, gx, fmaf(px, gy, pw * gz)));
    q[0] = xyzw ? ox : ow;
    q[1] = xyzw ? oy : ox;
    q[2] = xyzw ? oz : oy;
    q[3] = xyzw ? ow : oz;
}

// out = s^2 E S E^T for the entries (i, j) the form stores
template <bool FULL>
__device__ __forceinline__ void xf_cov(float* c, const float* __restrict__ T, bool bwd)
{
    const Xf x = load_xf(T, bwd);
    const float s2 = x.s * x.s;
    float S[9];
    if constexpr (FULL) {
#pragma unroll
        for (int k = 0; k < 9; ++k) S[k] = c[k];
    } else {
        // backward: the chains run on (g_xx, g_xy / 2, g_xz / 2, g_yy, g_yz / 2, g_zz)
        const float h = bwd ? 0.5f : 1.0f;
        S[0] = c[0]; S[1] = S[3] = h * c[1]; S[2] = S[6] = h * c[2]; S[4] = c[3]; S[5] = S[7] = h * c[4]; S[8] = c[5];
    }
    float Tm[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) Tm[i * 3 + k] = fmaf(x.E[i * 3 + 2], S[6 + k], fmaf(x.E[i * 3 + 1], S[3 + k], x.E[i * 3] * S[k]));
    int o = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = FULL ? 0 : i; j < 3; ++j) {
            const float y = s2 * fmaf(Tm[i * 3 + 2], x.E[j * 3 + 2], fmaf(Tm[i * 3 + 1], x.E[j * 3 + 1], Tm[i * 3] * x.E[j * 3]));
            c[o++] = (!FULL && bwd && i != j) ? 2.0f * y : y;
        }
}

// one array of W floats per Gaussian: the thread's run of four Gaussians through f(values of one Gaussian, row pointer)
template <int W, class F>
__device__ __forceinline__ void geom_array(const float* in, float* out, long long n0, int N, const int (&vid)[kGeomGroup],
                                           const float* __restrict__ table, F&& f)
{
    constexpr int S = kGeomGroup * W;
    const size_t total = (size_t)N * W, off = (size_t)n0 * W;
    float v[S];
    load_run<S>(in, off, total, aligned16(in), v);
#pragma unroll
    for (int j = 0; j < kGeomGroup; ++j) with_row(vid[j], table, [&](const float* __restrict__ T) { f(v + j * W, T); });
    store_run<S>(out, off, total, aligned16(out), v);
}

template <bool COV_FULL>
__global__ __launch_bounds__(kThreads) void geom_kernel(int N, int V, int bwd_, int xyzw_, const float* __restrict__ table,
                                                        const long long* __restrict__ ids, const float* means_in,
                                                        const float* scales_in, const float* rot_in, const float* cov_in,
                                                        float* means_out, float* scales_out, float* rot_out, float* cov_out)
{
    const long long n0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * kGeomGroup;
    if (n0 >= N) return;
    const bool bwd = bwd_ != 0, xyzw = xyzw_ != 0;
    int vid[kGeomGroup];
#pragma unroll
    for (int j = 0; j < kGeomGroup; ++j) vid[j] = row_of_gaussian(n0 + j, N, V, ids);
    if (means_in) geom_array<3>(means_in, means_out, n0, N, vid, table, [&](float* m, const float* __restrict__ T) { xf_mean(m, T, bwd); });
    if (scales_in) geom_array<3>(scales_in, scales_out, n0, N, vid, table, [&](float* s, const float* __restrict__ T) { xf_scale(s, T); });
    if (rot_in) geom_array<4>(rot_in, rot_out, n0, N, vid, table, [&](float* q, const float* __restrict__ T) { xf_quat(q, T, bwd, xyzw); });
    if (cov_in)
        geom_array<COV_FULL ? 9 : 6>(cov_in, cov_out, n0, N, vid, table,
                                     [&](float* c, const float* __restrict__ T) { xf_cov<COV_FULL>(c, T, bwd); });
}

// ---- the table ---------------------------------------------------------------------------------------------------------------

// the degree-7 Lebedev rule: 6 axes (weight 1/21), 12 edge midpoints (4/105), 8 corners (9/280); the weights sum to 1
constexpr double kA = 0.70710678118654752440, kB = 0.57735026918962576451;
__device__ constexpr double kNodes[26][3] = {
    {1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1},
    {0, kA, kA}, {0, kA, -kA}, {0, -kA, kA}, {0, -kA, -kA}, {kA, 0, kA}, {kA, 0, -kA}, {-kA, 0, kA}, {-kA, 0, -kA},
    {kA, kA, 0}, {kA, -kA, 0}, {-kA, kA, 0}, {-kA, -kA, 0},
    {kB, kB, kB}, {kB, kB, -kB}, {kB, -kB, kB}, {kB, -kB, -kB}, {-kB, kB, kB}, {-kB, kB, -kB}, {-kB, -kB, kB}, {-kB, -kB, -kB}};
constexpr double kFourPi = 12.566370614359172954;

// band L of the rasterizer's basis (fs_common.h sh_basis) in fp64, with the fp64 values of its constants
template <int L>
__device__ __forceinline__ void band_basis(double x, double y, double z, double* b)
{
    const double xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    if constexpr (L == 1) {
        constexpr double c1 = 0.4886025119029199;
        b[0] = -c1 * y; b[1] = c1 * z; b[2] = -c1 * x;
    } else if constexpr (L == 2) {
        b[0] = 1.0925484305920792 * xy;
        b[1] = -1.0925484305920792 * yz;
        b[2] = 0.31539156525252005 * (2.0 * zz - xx - yy);
        b[3] = -1.0925484305920792 * xz;
        b[4] = 0.5462742152960396 * (xx - yy);
    } else {
        b[0] = -0.5900435899266435 * y * (3.0 * xx - yy);
        b[1] = 2.890611442640554 * xy * z;
        b[2] = -0.4570457994644658 * y * (4.0 * zz - xx - yy);
        b[3] = 0.3731763325901154 * z * (2.0 * zz - 3.0 * xx - 3.0 * yy);
        b[4] = -0.4570457994644658 * x * (4.0 * zz - xx - yy);
        b[5] = 1.445305721320277 * z * (xx - yy);
        b[6] = -0.5900435899266435 * x * (xx - 3.0 * yy);
    }
}

// D_L = 4 pi sum_k w_k b_L(R d_k) b_L(d_k)^T, rounded once
template <int L>
__device__ __forceinline__ void band_matrix(const double (&R)[9], float* __restrict__ out)
{
    constexpr int n = 2 * L + 1;
    double D[n * n];
#pragma unroll
    for (int k = 0; k < n * n; ++k) D[k] = 0.0;
#pragma unroll 1
    for (int k = 0; k < 26; ++k) {
        const double x = kNodes[k][0], y = kNodes[k][1], z = kNodes[k][2];
        const double w = kFourPi * (k < 6 ? 1.0 / 21.0 : k < 18 ? 4.0 / 105.0 : 9.0 / 280.0);
        double b[n], br[n];
        band_basis<L>(x, y, z, b);
        band_basis<L>(R[0] * x + R[1] * y + R[2] * z, R[3] * x + R[4] * y + R[5] * z, R[6] * x + R[7] * y + R[8] * z, br);
#pragma unroll
        for (int i = 0; i < n; ++i)
#pragma unroll
            for (int j = 0; j < n; ++j) D[i * n + j] = fma(w * br[i], b[j], D[i * n + j]);
    }
#pragma unroll
    for (int k = 0; k < n * n; ++k) out[k] = (float)D[k];
}

__global__ __launch_bounds__(64) void prepare_kernel(int V, const float* __restrict__ xf, float* __restrict__ table)
{
    const int v = blockIdx.x * 64 + threadIdx.x;
    if (v >= V) return;
    const float* __restrict__ a = xf + (size_t)v * 12;
    float* __restrict__ T = table + (size_t)v * kRow;
    double A[9], R[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) A[i * 3 + j] = (double)a[i * 4 + j];
    const double det = A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6]);
    const double s = cbrt(det);
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = A[k] / s;
    // the nearest rotation (the polar factor) by Newton's iteration R <- (R + R^-T) / 2: the fp32 entries of xf are a rotation
    // only to 2^-24, the iteration squares that deviation per step, and q_R and D_l are then functions of an exact rotation
#pragma unroll 1
    for (int it = 0; it < 3; ++it) {
        const double C[9] = {R[4] * R[8] - R[5] * R[7], R[5] * R[6] - R[3] * R[8], R[3] * R[7] - R[4] * R[6],
                             R[2] * R[7] - R[1] * R[8], R[0] * R[8] - R[2] * R[6], R[1] * R[6] - R[0] * R[7],
                             R[1] * R[5] - R[2] * R[4], R[2] * R[3] - R[0] * R[5], R[0] * R[4] - R[1] * R[3]};   // cofactors: det R^-T
        const double d = R[0] * C[0] + R[1] * C[1] + R[2] * C[2];
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = 0.5 * (R[k] + C[k] / d);
    }
    T[FS_TRANSFORM_S] = (float)s;
#pragma unroll
    for (int k = 0; k < 9; ++k) T[FS_TRANSFORM_R + k] = (float)R[k];
#pragma unroll
    for (int i = 0; i < 3; ++i) T[FS_TRANSFORM_T + i] = a[i * 4 + 3];
    // four candidate quaternions, each exact where its own component is the largest; take that one
    const double t0 = 1.0 + R[0] + R[4] + R[8], t1 = 1.0 + R[0] - R[4] - R[8], t2 = 1.0 - R[0] + R[4] - R[8], t3 = 1.0 - R[0] - R[4] + R[8];
    double q[4];
    if (t0 >= t1 && t0 >= t2 && t0 >= t3) {
        q[0] = t0; q[1] = R[7] - R[5]; q[2] = R[2] - R[6]; q[3] = R[3] - R[1];
    } else if (t1 >= t2 && t1 >= t3) {
        q[0] = R[7] - R[5]; q[1] = t1; q[2] = R[3] + R[1]; q[3] = R[2] + R[6];
    } else if (t2 >= t3) {
        q[0] = R[2] - R[6]; q[1] = R[3] + R[1]; q[2] = t2; q[3] = R[7] + R[5];
    } else {
        q[0] = R[3] - R[1]; q[1] = R[2] + R[6]; q[2] = R[7] + R[5]; q[3] = t3;
    }
    const double nq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double sg = q[0] < 0.0 ? -1.0 / nq : 1.0 / nq;
#pragma unroll
    for (int k = 0; k < 4; ++k) T[FS_TRANSFORM_Q + k] = (float)(q[k] * sg);
    band_matrix<1>(R, T + FS_TRANSFORM_D1);
    band_matrix<2>(R, T + FS_TRANSFORM_D2);
    band_matrix<3>(R, T + FS_TRANSFORM_D3);
}

bool valid_m(int32_t M) { return M == 1 || M == 4 || M == 9 || M == 16; }

template <int M>
void launch_sh(int32_t N, int32_t V, int32_t flags, const float* in, const float* table, const int64_t* ids, float* out, hipStream_t st)
{
    const long long units = ((long long)N + ShRun<M>::G - 1) / ShRun<M>::G;
    const dim3 grid((unsigned)((units + kThreads - 1) / kThreads)), block(kThreads);
    const int tr = (flags & FS_TRANSFORM_SH_TRANSPOSE) ? 1 : 0;
    if (flags & FS_TRANSFORM_SH_CHANNEL_MAJOR)
        hipLaunchKernelGGL((sh_rotate_kernel<M, true>), grid, block, 0, st, N, V, tr, in, table, (const long long*)ids, out);
    else
        hipLaunchKernelGGL((sh_rotate_kernel<M, false>), grid, block, 0, st, N, V, tr, in, table, (const long long*)ids, out);
}

// M = 1 in place has nothing to do (band 0 does not rotate); every other case is one launch
void rotate_sh(int32_t N, int32_t M, int32_t V, int32_t flags, const float* in, const float* table, const int64_t* ids, float* out,
               hipStream_t st)
{
    switch (M) {
        case 1:
            if (in != out) launch_sh<1>(N, V, flags, in, table, ids, out, st);
            break;
        case 4: launch_sh<4>(N, V, flags, in, table, ids, out, st); break;
        case 9: launch_sh<9>(N, V, flags, in, table, ids, out, st); break;
        default: launch_sh<16>(N, V, flags, in, table, ids, out, st); break;
    }
}

int transform(bool bwd, int32_t N, int32_t M, int32_t V, int32_t flags, const float* table, const int64_t* ids, const float* means_in,
              const float* scales_in, const float* rot_in, const float* cov_in, const float* shs_in, float* means_out,
              float* scales_out, float* rot_out, float* cov_out, float* shs_out, void* stream_)
{
    if (N <= 0 || V <= 0 || !valid_m(M) || !table || (!ids && V != 1) || (flags & ~kFlagMask) || (flags & FS_TRANSFORM_SH_TRANSPOSE))
        return FS_ERR_INVALID_ARG;
    if (!means_in && !scales_in && !rot_in && !cov_in && !shs_in) return FS_ERR_INVALID_ARG;
    if ((means_in && !means_out) || (scales_in && !scales_out) || (rot_in && !rot_out) || (cov_in && !cov_out) || (shs_in && !shs_out))
        return FS_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream_;
    if (means_in || scales_in || rot_in || cov_in) {
        const long long units = ((long long)N + kGeomGroup - 1) / kGeomGroup;
        const dim3 grid((unsigned)((units + kThreads - 1) / kThreads)), block(kThreads);
        const int xyzw = (flags & FS_TRANSFORM_QUAT_XYZW) ? 1 : 0;
        if (flags & FS_TRANSFORM_COV_FULL)
            hipLaunchKernelGGL((geom_kernel<true>), grid, block, 0, st, N, V, bwd ? 1 : 0, xyzw, table, (const long long*)ids, means_in,
                               scales_in, rot_in, cov_in, means_out, scales_out, rot_out, cov_out);
        else
            hipLaunchKernelGGL((geom_kernel<false>), grid, block, 0, st, N, V, bwd ? 1 : 0, xyzw, table, (const long long*)ids, means_in,
                               scales_in, rot_in, cov_in, means_out, scales_out, rot_out, cov_out);
    }
    if (shs_in) rotate_sh(N, M, V, (flags & FS_TRANSFORM_SH_CHANNEL_MAJOR) | (bwd ? FS_TRANSFORM_SH_TRANSPOSE : 0), shs_in, table, ids, shs_out, st);
    return FS_OK;
}

}  // namespace

}  // namespace fs

using namespace fs;

FS_API int fs_transform_api_version(void) { return FS_TRANSFORM_API_VERSION; }

FS_API int fs_transform_prepare(int32_t V, const float* xf, float* table, void* stream_)
{
    if (V <= 0 || !xf || !table) return FS_ERR_INVALID_ARG;
    hipLaunchKernelGGL(prepare_kernel, dim3((unsigned)((V + 63) / 64)), dim3(64), 0, (hipStream_t)stream_, V, xf, table);
    FS_CHECK_LAUNCH("transform_prepare");
    return FS_OK;
}

FS_API int fs_sh_rotate(int32_t N, int32_t M, int32_t V, int32_t flags, const float* sh_in, const float* table, const int64_t* ids,
                        float* sh_out, void* stream_)
{
    if (N <= 0 || V <= 0 || !valid_m(M) || !sh_in || !table || !sh_out || (!ids && V != 1) ||
        (flags & ~(FS_TRANSFORM_SH_CHANNEL_MAJOR | FS_TRANSFORM_SH_TRANSPOSE)))
        return FS_ERR_INVALID_ARG;
    rotate_sh(N, M, V, flags, sh_in, table, ids, sh_out, (hipStream_t)stream_);
    FS_CHECK_LAUNCH("sh_rotate");
    return FS_OK;
}

FS_API int fs_gaussians_transform_forward(int32_t N, int32_t M, int32_t V, int32_t flags, const float* table, const int64_t* ids,
                                          const float* means_in, const float* scales_in, const float* rotations_in,
                                          const float* cov_in, const float* shs_in, float* means_out, float* scales_out,
                                          float* rotations_out, float* cov_out, float* shs_out, void* stream_)
{
    if (const int st = transform(false, N, M, V, flags, table, ids, means_in, scales_in, rotations_in, cov_in, shs_in, means_out,
                                 scales_out, rotations_out, cov_out, shs_out, stream_))
        return st;
    FS_CHECK_LAUNCH("gaussians_transform_forward");
    return FS_OK;
}

FS_API int fs_gaussians_transform_backward(int32_t N, int32_t M, int32_t V, int32_t flags, const float* table, const int64_t* ids,
                                           const float* g_means_out, const float* g_scales_out, const float* g_rotations_out,
                                           const float* g_cov_out, const float* g_shs_out, float* g_means_in, float* g_scales_in,
                                           float* g_rotations_in, float* g_cov_in, float* g_shs_in, void* stream_)
{
    if (const int st = transform(true, N, M, V, flags, table, ids, g_means_out, g_scales_out, g_rotations_out, g_cov_out, g_shs_out,
                                 g_means_in, g_scales_in, g_rotations_in, g_cov_in, g_shs_in, stream_))
        return st;
    FS_CHECK_LAUNCH("gaussians_transform_backward");
    return FS_OK;
}
