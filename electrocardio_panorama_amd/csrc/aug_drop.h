// The lead-drop decision of the input augmentation (nef_augment_args, include/nefnet_hip.h): whether row (b, v) is zeroed.  One
// definition for augment.hip, which zeroes the row, and lead_mask.hip, which writes the mask the head reads (nef_augment_mask).
#pragma once
#include "nef_common.h"

namespace nef_aug {

constexpr float INV24F = 1.0f / 16777216.0f;
constexpr uint64_t ROW_BASE = 1ull << 62;       // row counters live far above every element counter

__device__ __forceinline__ uint32_t field0(uint64_t z) { return (uint32_t)(z >> 40); }
__device__ __forceinline__ uint32_t field1(uint64_t z) { return (uint32_t)((z >> 16) & 0xFFFFFFull); }

// row (b, v) of V drew "dropped" -- and is kept all the same when every lead of the sample did and it is the fallback lead
__device__ __forceinline__ bool lead_dropped(uint64_t seed, int b, int v, int V, float lead_drop) {
    if (!(lead_drop > 0.f)) return false;
    if (!(field1(nef_rng_mix(seed, ROW_BASE + 4ull * (uint64_t)(b * V + v) + 2)) * INV24F < lead_drop)) return false;
    bool all = true;
    for (int v2 = 0; v2 < V; ++v2)
        all = all && field1(nef_rng_mix(seed, ROW_BASE + 4ull * (uint64_t)(b * V + v2) + 2)) * INV24F < lead_drop;
    const int fallback = (int)(((uint64_t)V * field0(nef_rng_mix(seed, ROW_BASE + 4ull * (uint64_t)(b * V) + 3))) >> 24);
    return !(all && fallback == v);
}

}  // namespace nef_aug
