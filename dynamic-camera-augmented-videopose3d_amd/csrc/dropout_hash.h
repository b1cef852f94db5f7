// The dropout keep mask of the training kernels (train.hip, seq_train.hip): counter-based
// (splitmix64 of seed, site, element), so a backward regenerates the mask instead of storing it.
// `site` is the conv layer of the temporal trainer, the mask site of the sequence trainer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vp3d {

__device__ __forceinline__ bool drop_keep(uint64_t seed, int layer, int64_t idx, uint64_t thresh) {
    uint64_t z = seed + (uint64_t)(layer + 1) * 0x9E3779B97F4A7C15ull + (uint64_t)idx * 0xD1B54A32D192ED03ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (z >> 32) < thresh;
}

// keep iff the hash's upper 32 bits < thresh; 2^32 = keep everything (p = 0: the hash is skipped)
inline uint64_t keep_threshold(float p) {
    if (p <= 0.f) return 1ull << 32;
    const double keep = 1.0 - (double)p;
    return (uint64_t)(keep * 4294967296.0);
}

inline float keep_scale(float p) { return p > 0.f ? 1.0f / (float)(1.0 - (double)p) : 1.0f; }

}  // namespace vp3d
