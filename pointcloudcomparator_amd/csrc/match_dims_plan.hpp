// match_dims_plan.hpp -- the host side of pcc_match_knn_batch_dims for dim != 3 (match_dims.hip): the packed record, and
// match_plan.hpp's plan at this record's slice.  Plain C++ (no HIP): tests/cpp/test_match_dims_plan.cpp compiles it on its own.
//
// The record: DP floats, DP = the smallest of 4, 8, 16, 32 that holds `dim`; floats dim .. DP-1 are +0.  A padded term of the
// distance is (0 - 0) * (0 - 0) = +0 and d + 0 == d for every d >= 0 and for +inf, so the padded sum has the bits of the sum
// over `dim` terms.  A record whose first `dim` floats are not all finite (PCL's isValid over nr_dimensions) is packed as
// (+inf, 0, ... 0): its distance to every valid record is +inf and to another invalid one NaN, both "no neighbour" by
// key_none -- the kernel needs no test on the record, and neither side of such a pair is ever reported.
//
// The table of work items is match_plan.hpp's, its slice at most match_dims_slice_max(DP).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <limits>

#include "match_plan.hpp"

namespace pcc {

constexpr int MD_DIM_MAX = 32;

// the padded record width: the smallest of 4, 8, 16, 32 that is >= dim (dim in 1 .. 32)
inline int match_dims_padded(int dim) { return dim <= 4 ? 4 : dim <= 8 ? 8 : dim <= 16 ? 16 : 32; }

// n records of `stride` bytes -> n records of dp floats at `out`.  Reads 4 * dim bytes of every record and no more (the last
// record of an array may end there).  Returns the number of valid records.
inline size_t match_dims_pack(const void* raw, size_t n, size_t stride, int dim, int dp, float* out) {
    const char* p = static_cast<const char*>(raw);
    size_t valid_n = 0;
    float v[MD_DIM_MAX];
    for (size_t i = 0; i < n; ++i, out += dp) {
        memcpy(v, p + i * stride, 4 * (size_t)dim);
        bool valid = true;
        for (int k = 0; k < dim; ++k) valid = valid && (v[k] - v[k]) == 0.0f;  // (finite: neither NaN nor +-inf)
        for (int k = 0; k < dp; ++k) out[k] = (valid && k < dim) ? v[k] : 0.0f;
        if (!valid) out[0] = std::numeric_limits<float>::infinity();
        valid_n += valid ? 1 : 0;
    }
    return valid_n;
}

using MatchDimsPlan = MatchPlan;

// Lays the records out and builds the table.  false: more than 2^31 - 1 records or items (nothing usable in *plan).
inline bool match_dims_plan(size_t n_pairs, const void* const* des1, const size_t* n1, const size_t* n2, int dp, MatchDimsPlan* plan) {
    return match_plan(n_pairs, des1, n1, n2, match_dims_slice_max(dp), plan);
}

}  // namespace pcc
