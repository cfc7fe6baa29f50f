// match_fpfh_plan.hpp -- the host side of pcc_match_fpfh_batch (match_fpfh.hip): the packed record, the table the pack from device
// memory is driven by, and match_plan.hpp's plan at this record's slice.  Plain C++ (no HIP): tests/cpp/test_match_fpfh_plan.cpp
// compiles it on its own.
//
// The record: MF_DP = 36 floats, the 33 bins of a pcl::FPFHSignature33 and three +0.  144 bytes is a multiple of 16: the float4 loads
// of match_load_query and the wave-uniform loads of the references stay aligned.  The padding argument of match_dims_plan.hpp holds:
// a padded term is (0 - 0) * (0 - 0) = +0 and d + 0 == d for every d >= 0 and for +inf.  A record whose 33 floats are not all finite
// is packed as (+inf, 0, ... 0): +inf from every valid record and NaN from another invalid one, both "no neighbour" by key_none.
//
// The table of work items is match_plan.hpp's, its slice at most match_dims_slice_max(36) = 512.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <limits>
#include <vector>

#include "match_plan.hpp"

namespace pcc {

constexpr int MF_DIM = 33;  // the bins read of every record
constexpr int MF_DP = 36;   // floats of a packed record

// n records of `stride` bytes -> n records of MF_DP floats at `out`.  Reads 132 bytes of every record and no more (the last record
// of an array may end there).  Returns the number of valid records.
inline size_t match_fpfh_pack(const void* raw, size_t n, size_t stride, float* out) {
    const char* p = static_cast<const char*>(raw);
    size_t valid_n = 0;
    float v[MF_DIM];
    for (size_t i = 0; i < n; ++i, out += MF_DP) {
        memcpy(v, p + i * stride, 4 * (size_t)MF_DIM);
        bool valid = true;
        for (int k = 0; k < MF_DIM; ++k) valid = valid && (v[k] - v[k]) == 0.0f;  // (finite: neither NaN nor +-inf)
        for (int k = 0; k < MF_DP; ++k) out[k] = (valid && k < MF_DIM) ? v[k] : 0.0f;
        if (!valid) out[0] = std::numeric_limits<float>::infinity();
        valid_n += valid ? 1 : 0;
    }
    return valid_n;
}

using MatchFpfhPlan = MatchPlan;

// Lays the records out and builds the table.  false: more than 2^31 - 1 records or items (nothing usable in *plan).
inline bool match_fpfh_plan(size_t n_pairs, const void* const* des1, const size_t* n1, const size_t* n2, MatchFpfhPlan* plan) {
    return match_plan(n_pairs, des1, n1, n2, match_dims_slice_max(MF_DP), plan);
}

// One array of strided records in device memory and where its packed records go: records rec0 .. rec0 + n - 1 of the call.
struct MatchFpfhSource {
    const void* p;
    uint32_t n, rec0;
};

// The arrays the pack kernel reads: every distinct des1 once, then every des2, in the order of their packed records; none of them
// empty, so the rec0 ascend strictly from 0 and every packed record lies in exactly one source.
inline void match_fpfh_sources(const MatchFpfhPlan& plan, size_t n_pairs, const void* const* des2, const size_t* n2,
                               std::vector<MatchFpfhSource>* sources) {
    sources->clear();
    for (const MatchFpfhPlan::Cloud& c : plan.clouds)
        if (c.n) sources->push_back({c.p, (uint32_t)c.n, (uint32_t)c.rec0});
    for (size_t p = 0; p < n_pairs; ++p)
        if (n2[p]) sources->push_back({des2[p], (uint32_t)n2[p], (uint32_t)plan.q_rec0[p]});
}

}  // namespace pcc
