// gsx_wave.h — cross-lane helpers of a 64-lane wave, shared by the kernels
// that count the columns of a bit matrix (gsx_prop_stats.hip,
// gsx_prop_traffic.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsx {

// Lane l gives row l of a 64 x 64 bit matrix and gets column l (bit k of the
// result: bit l of lane k's x).  Step s swaps the off-diagonal s x s blocks.
__device__ __forceinline__ uint64_t wave_transpose64(uint64_t x, uint32_t lane) {
    constexpr uint64_t M[6] = {0x5555555555555555ull, 0x3333333333333333ull, 0x0F0F0F0F0F0F0F0Full,
                               0x00FF00FF00FF00FFull, 0x0000FFFF0000FFFFull, 0x00000000FFFFFFFFull};
#pragma unroll
    for (int j = 5; j >= 0; --j) {
        const uint32_t s = 1u << j;
        const uint64_t m = M[j];  // the bits b with (b & s) == 0
        const uint64_t y = __shfl_xor(x, (int)s);
        x = (lane & s) ? ((x & ~m) | ((y >> s) & m)) : ((x & m) | ((y & m) << s));
    }
    return x;
}

__device__ __forceinline__ uint64_t read_lane64(uint64_t v, uint32_t l) {  // l wave-uniform
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l);
    return ((uint64_t)hi << 32) | lo;
}

}  // namespace gsx
