// sr_spot_dev.h -- the packed (cost, start) state of the subsequence DTW kernels (k_spot.hip, k_chain.hip): cost in the high
// word of one u64, so that the tie rule (smallest start among equal costs) is the u64 minimum; unreachable = all ones.
// gfx950 (MI355X, CDNA4) only; wave = 64 lanes.
#pragma once
#include "sr_dtw_dev.h"

namespace sr {

constexpr uint64_t kSpotInf = ~0ull;

__device__ __forceinline__ uint64_t spot_min(uint64_t a, uint64_t b) { return b < a ? b : a; }
__device__ __forceinline__ uint64_t spot_add(uint64_t a, uint32_t d) { return a == kSpotInf ? kSpotInf : a + ((uint64_t)d << 32); }
__device__ __forceinline__ uint64_t spot_shfl_up(uint64_t v, uint32_t by)
{
    const uint32_t lo = __shfl_up((uint32_t)v, by, 64), hi = __shfl_up((uint32_t)(v >> 32), by, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t spot_shfl(uint64_t v, uint32_t from)
{
    const uint32_t lo = __shfl((uint32_t)v, (int)from, 64), hi = __shfl((uint32_t)(v >> 32), (int)from, 64);
    return ((uint64_t)hi << 32) | lo;
}

}  // namespace sr
