// knn_merge.hpp -- the merge network of the wave-cooperative k-NN kernels (gfx950): a running top list of 64 * KR keys, one to
// KR registers per lane, ascending over (register, lane), and the batch of 64 keys that is folded into it (knn.hip's selection
// by a wave per query over the grid; region_rgb_batch.hip's segmented rows over LDS tiles).  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include "lane_ops.hpp"

namespace pcc {

// value of lane `src`; src must be wave-uniform (v_readlane_b32)
__device__ __forceinline__ unsigned long long shfl_u64(unsigned long long v, int src) {
    const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)v, src);
    const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long cmpx(unsigned long long v, int m, bool take_min, unsigned int lane) {
    const unsigned long long o = xor_lane_u64(v, m, lane);
    const bool o_less = o < v;
    return (o_less == take_min) ? o : v;
}
__device__ __forceinline__ unsigned long long bitonic_sort64(unsigned long long v, unsigned int lane) {
#pragma unroll
    for (int k2 = 2; k2 <= 64; k2 <<= 1)
#pragma unroll
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            const bool up = (lane & k2) == 0, lower = (lane & j) == 0;
            v = cmpx(v, j, lower == up, lane);
        }
    return v;  // ascending over the lanes
}
__device__ __forceinline__ unsigned long long bitonic_merge64(unsigned long long v, unsigned int lane) {
#pragma unroll
    for (int j = 32; j > 0; j >>= 1) v = cmpx(v, j, (lane & j) == 0, lane);
    return v;  // bitonic in -> ascending out
}

// merge a batch of 64 keys into the sorted top list (64 * KR keys, ascending over (register, lane)): the sorted
// batch enters register 0; what each register pushes out (the upper half of a 128-key bitonic split) cascades
// into the next one; the overflow of the last register is dropped
template <int KR>
__device__ __forceinline__ void topk_merge(unsigned long long (&top)[KR], unsigned long long batch, unsigned int lane) {
    unsigned long long carry = bitonic_sort64(batch, lane);
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const unsigned long long rev = reverse_lanes_u64(carry, lane);
        const unsigned long long lo = rev < top[r] ? rev : top[r];
        const unsigned long long hi = rev < top[r] ? top[r] : rev;
        top[r] = bitonic_merge64(lo, lane);
        if (r + 1 < KR) carry = bitonic_merge64(hi, lane);
    }
}

}  // namespace pcc
