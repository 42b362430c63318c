// The one LDS scan of the MSM's entries stage (msm_entries.hip), in a header of its own so that tests/cpp/scantest.hip can call it by itself.
#pragma once
#include <cstdint>

#include "zk_defs.hpp"

#if defined(__HIPCC__)  // device code only
namespace zkhip {

// sum over the 64 lanes of a wave, in every lane
ZK_D uint32_t wave_sum(uint32_t x) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

// Inclusive scan over one LDS word per lane, in place; every lane has written its own word.  Two barriers: a shuffle scan inside
// each wave, the (<= 16) wave totals through LDS, every lane adds the totals of the waves below its own.  After the call each lane
// may read any word of `scratch`; a barrier has to stand between those reads and the next write to `scratch`.
template <uint32_t THREADS>
ZK_D void block_inclusive_scan(uint32_t *scratch) {
    constexpr uint32_t WAVES = THREADS / 64;
    static_assert(THREADS % 64 == 0 && WAVES <= 16, "one LDS word per wave total, at most 16 of them");
    __shared__ uint32_t wave_total[WAVES];
    const uint32_t t = threadIdx.x, lane = t & 63, wave = t >> 6;
    uint32_t x = scratch[t];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= (uint32_t)d) x += y;
    }
    if (lane == 63) wave_total[wave] = x;
    __syncthreads();
    uint32_t below = 0;
#pragma unroll
    for (uint32_t k = 0; k + 1 < WAVES; ++k) below += k < wave ? wave_total[k] : 0u;
    scratch[t] = x + below;
    __syncthreads();
}

}  // namespace zkhip
#endif
