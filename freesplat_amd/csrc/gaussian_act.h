// gaussian_act.h -- device functions shared by gaussian_adam.hip and gaussian_density.hip.
//
// The activations of the raw Gaussian parameters: the Adam step (before the update, for the chain rule; after it, for the
// outputs), fs_gaussian_activate and the density-control kernels all call these two, so one raw value gives one bit pattern
// everywhere.  Both translation units are compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/freesplat_amd_optim.h"

namespace fs {

__device__ __forceinline__ float act_scale(float x) { return expf(x); }
__device__ __forceinline__ float act_opacity(float x) { return 1.0f / (1.0f + expf(-x)); }

// Floats per row of array KIND (FS_OPTIM_*), and the split of a flat element index into (row, position in the row).
template <int KIND>
__device__ __forceinline__ uint32_t row_width(int M)
{
    return KIND == FS_OPTIM_OPACITIES ? 1u : KIND == FS_OPTIM_ROTATIONS ? 4u : KIND == FS_OPTIM_SHS ? 3u * (uint32_t)M : 3u;
}

// i = q * width + r, with the division by a constant in every branch
template <int KIND>
__device__ __forceinline__ void row_of(uint32_t i, int M, uint32_t& q, uint32_t& r)
{
    if constexpr (KIND == FS_OPTIM_OPACITIES) {
        q = i; r = 0;
    } else if constexpr (KIND == FS_OPTIM_ROTATIONS) {
        q = i >> 2; r = i & 3u;
    } else if constexpr (KIND != FS_OPTIM_SHS) {
        q = i / 3u; r = i - 3u * q;
    } else {
        switch (M) {
            case 1: q = i / 3u; r = i - 3u * q; break;
            case 4: q = i / 12u; r = i - 12u * q; break;
            case 9: q = i / 27u; r = i - 27u * q; break;
            default: q = i / 48u; r = i - 48u * q; break;
        }
    }
}

// The generator of the split offsets (include/freesplat_amd_density.h): a pure function of (seed, source row, child, word) in
// wrapping 32-bit arithmetic -- murmur3's finaliser, chained -- so a uint32 restatement reproduces its bits.
__host__ __device__ __forceinline__ uint32_t density_fmix(uint32_t h)
{
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
__host__ __device__ __forceinline__ uint32_t density_bits(uint32_t seed, uint32_t row, uint32_t child, uint32_t word)
{
    return density_fmix(density_fmix(density_fmix(seed ^ 0x9E3779B9u) ^ row) + 0x9E3779B1u * (8u * child + word + 1u));
}
// u in (0, 1]: 24 bits, the half-step offset keeps 0 out (the fp32 sum is exact below 2^23 and rounds to even above)
__host__ __device__ __forceinline__ float density_uniform(uint32_t bits) { return ((float)(bits >> 8) + 0.5f) * 5.9604644775390625e-08f; }
// component c of the three standard normals of (seed, row, child): Box-Muller in fp32, words 2c and 2c + 1
__device__ __forceinline__ float density_normal(uint32_t seed, uint32_t row, uint32_t child, uint32_t c)
{
    const float u1 = density_uniform(density_bits(seed, row, child, 2u * c));
    const float u2 = density_uniform(density_bits(seed, row, child, 2u * c + 1u));
    return sqrtf(-2.0f * logf(u1)) * cosf(6.2831855f * u2);
}

}  // namespace fs
