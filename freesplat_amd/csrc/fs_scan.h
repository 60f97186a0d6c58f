// fs_scan.h -- device helpers of the order-preserving compactions ("count, scan the block counts, emit in order"): ptf.hip,
// gaussian_density.hip, tsdf.hip and the deterministic rasterizer backward's inverted index (raster_bwd.hip).  A new op that
// compacts starts from these, not from a copy of another op's scan (DESIGN.md "Helper headers").  The count kernels' tail (a
// workgroup's total) is fs_reduce.h's wave_sum + waves_total.
//
// Integer arithmetic throughout: any correct form gives the same values, so nothing here carries a bit-level claim.
//
//   wave_incl_scan   inclusive scan over the 64 lanes of a wavefront, six __shfl_up steps.  No LDS.
//   block_excl_scan  exclusive scan over a workgroup of 256 threads: the wave scan, the four wave totals through LDS, ONE
//                    barrier.  LDS [4] uint32.
//   slice_scan       exclusive scan of any number of counts by ONE workgroup of kScanThreads = 1024 threads.  LDS [1024] T.
//   load_flags4 / store_flags4   four consecutive byte flags as one uint32, a dword access where it is possible.
#pragma once
#include "fs_common.h"

namespace fs {

constexpr int kScanThreads = 1024;                           // threads of slice_scan's workgroup

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
    const uint32_t lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int s = 1; s < kWave; s <<= 1) {
        const uint32_t o = __shfl_up(v, s, kWave);
        if (lane >= (uint32_t)s) v += o;
    }
    return v;
}

// The number of items of the threads before this one (x summed over the lower thread indices) in a workgroup of 256 threads;
// total = the workgroup's sum, valid in every thread.  There is NO barrier after the reads of s_w: a caller that calls this in
// a loop with the same s_w ends its loop body with a __syncthreads() of its own (det_scan_totals_kernel), a caller that calls
// it once pays for nothing.
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t x, uint32_t* s_w /* [4] */, uint32_t& total)
{
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const uint32_t inc = wave_incl_scan(x);
    if (lane == kWave - 1) s_w[wave] = inc;
    __syncthreads();
    uint32_t wave_off = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k)
        if (k < wave) wave_off += s_w[k];
    total = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
    return wave_off + inc - x;
}

__device__ __forceinline__ uint32_t block_excl_scan(uint32_t x, uint32_t* s_w /* [4] */)
{
    uint32_t total;
    return block_excl_scan(x, s_w, total);
}

// ONE workgroup of kScanThreads threads: out[k] = counts[0] + .. + counts[k - 1] for k < n, in T (uint32_t, or unsigned long
// long where the sum may pass 2^32).  Thread t owns the contiguous slice of ceil(n / 1024) counts that starts at t times that,
// so any n is covered: the slices' sums are scanned in part[] (Hillis-Steele), then each thread runs through its slice.
// out may be counts itself (T = uint32_t: in place), hence no __restrict__; out == nullptr writes nothing ("sum only").
// Returns the sum of the slices of threads 0 .. t: the sum of ALL counts in the LAST thread (t == kScanThreads - 1), which is
// the one that stores it.  After the scan's last barrier a thread reads no slot of part[] but its own, so a kernel may call
// this again with the same part[] without a barrier in between.
template <class T>
__device__ __forceinline__ T slice_scan(const uint32_t* counts, uint32_t n, T* out, T* part /* [kScanThreads] */)
{
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n + kScanThreads - 1u) / kScanThreads;
    const uint32_t lo = min(n, t * per), hi = min(n, lo + per);
    T s = 0;
    for (uint32_t k = lo; k < hi; ++k) s += counts[k];
    part[t] = s;
    __syncthreads();
    for (uint32_t off = 1; off < (uint32_t)kScanThreads; off <<= 1) {
        const T v = (t >= off) ? part[t - off] : (T)0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    if (out) {
        T run = part[t] - s;
        for (uint32_t k = lo; k < hi; ++k) {
            const uint32_t c = counts[k];
            out[k] = run;
            run += c;
        }
    }
    return part[t];
}

// The four byte flags f[base .. base + 3] as one uint32, flag k in bits [8 k, 8 k + 8): one dword access when all four lie
// below n and the address is 4-byte aligned, byte accesses otherwise.  A byte at or past n reads as 0 and is not written; the
// store writes each byte as given.
__device__ __forceinline__ uint32_t load_flags4(const uint8_t* __restrict__ f, uint32_t base, uint32_t n)
{
    uint32_t v = 0;
    if (base + 3u < n && (((uintptr_t)(f + base)) & 3u) == 0) {
        v = *reinterpret_cast<const uint32_t*>(f + base);
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            if (base + k < n) v |= (uint32_t)f[base + k] << (8u * k);
    }
    return v;
}

__device__ __forceinline__ void store_flags4(uint8_t* __restrict__ f, uint32_t base, uint32_t n, uint32_t v)
{
    if (base + 3u < n && (((uintptr_t)(f + base)) & 3u) == 0) {
        *reinterpret_cast<uint32_t*>(f + base) = v;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            if (base + k < n) f[base + k] = (uint8_t)(v >> (8u * k));
    }
}

}  // namespace fs
