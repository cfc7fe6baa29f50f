// match_search.hpp -- the device scaffold of the descriptor searches (gfx950): k_match_batch (match_batch.hip), k_match_dims
// (match_dims.hip) and k_cm_search (cluster_match.hip) are one workgroup shape over match_plan.hpp's work items -- 64 queries, one
// per lane; MATCH_WAVES waves that each take a share of the item's slice of references through wave-uniform (scalar) loads;
// their partial minima meeting in LDS; the slices of a query block merging in device memory.  What is the same in all three is
// here.  What a kernel tracks per query (key and second minimum, or the distance alone), its loop with its pragmas, its launch
// bounds and its LDS arrays are its own: the loops differ in what they carry from one reference to the next, and the compiler's
// register allocation under the 64-VGPR bound was settled per loop (cluster_match.hip has the measured case).  The distance chain
// d = d0 * d0; d = d + d1 * d1; ... stays written out inside k_match_dims' and k_cm_search's loops for the same reason: behind a
// __forceinline__ function of (q, r) the same chain was scheduled differently and came out one VGPR lower at DP = 8 and 16 --
// another kernel than the measured one, with nothing to say which is faster.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

#include "match_plan.hpp"

namespace pcc {

constexpr int MATCH_WAVES = 16;  // waves of a workgroup: each takes a sixteenth of the slice for the same 64 queries

// who a thread is in its item: its lane = its query, its wave (uniform: the loop bounds and the references' addresses are
// scalars), and whether the item has a query for the lane at all
struct MatchLane {
    unsigned int lane, wave;
    bool live;
};
__device__ __forceinline__ MatchLane match_lane(const MatchItem& it) {
    const unsigned int lane = threadIdx.x & 63;
    return {lane, (unsigned int)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane < it.nq};
}

// the wave's share [b0, b1) of the item's nr references
struct MatchShare {
    unsigned int b0, b1;
};
__device__ __forceinline__ MatchShare match_share(unsigned int nr, unsigned int wave) {
    const unsigned int per = (nr + MATCH_WAVES - 1) / MATCH_WAVES;
    const unsigned int b0 = min(nr, wave * per);
    return {b0, min(nr, b0 + per)};
}

// the lane's query of DP floats (a lane without a query computes with the item's first one and reports nothing)
template <int DP>
__device__ __forceinline__ void match_load_query(const float* rec, const MatchItem& it, const MatchLane& me, float (&q)[DP]) {
    const float4* __restrict__ qp = reinterpret_cast<const float4*>(rec + (size_t)(it.q0 + (me.live ? me.lane : 0u)) * DP);
#pragma unroll
    for (int k = 0; k < DP / 4; ++k) {
        const float4 v = qp[k];
        q[4 * k] = v.x; q[4 * k + 1] = v.y; q[4 * k + 2] = v.z; q[4 * k + 3] = v.w;
    }
}

// f(std::integral_constant<int, DP>) for the padded record width dp = 4, 8, 16 or 32 (match_dims_padded)
template <class F>
inline void dispatch_dp(int dp, F&& f) {
    switch (dp) {
        case 4: f(std::integral_constant<int, 4>()); break;
        case 8: f(std::integral_constant<int, 8>()); break;
        case 16: f(std::integral_constant<int, 16>()); break;
        default: f(std::integral_constant<int, 32>()); break;
    }
}

}  // namespace pcc
