// fpfh_batch_plan.hpp -- the host-built tables of pcc_fpfh_descriptors_batch (fpfh_batch.hip).
// Plain C++ (no HIP): tests/cpp/test_fpfh_batch_plan.cpp compiles it on its own.
//
// The clusters of a call are ranges of ONE array of records: cluster c is records offsets[c] .. offsets[c + 1].  The clusters
// of up to `limit` points form the concatenation the batch kernels run over (bases and work items as rift_batch_plan builds
// them: a cluster off that route has size 0 there and shares its base with the cluster behind it); the larger ones take the
// single path on the work handle, one by one.  Once the slice bounds of the batch route and the row counts of the work handle
// are known, fpfh_batch_splice puts both back into cluster order: the caller's bounds, and the row copies that move the batch
// route's rows to their places.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "rift_batch_plan.hpp"

namespace pcc {

// what the offsets of a call are refused for, in this order: any decrease first, then the size
enum : int { FB_OFFSETS_OK = 0, FB_OFFSETS_DECREASE = 1, FB_OFFSETS_TOO_MANY = 2 };
// *bad (nullable): the first cluster whose end lies in front of its start
inline int fpfh_batch_check_offsets(const size_t* offsets, size_t n_clusters, size_t* bad = nullptr) {
    for (size_t c = 0; c < n_clusters; ++c)
        if (offsets[c + 1] < offsets[c]) {
            if (bad) *bad = c;
            return FB_OFFSETS_DECREASE;
        }
    if (n_clusters >= (1ull << 31) || (n_clusters && offsets[n_clusters] - offsets[0] >= (1ull << 31))) return FB_OFFSETS_TOO_MANY;
    return FB_OFFSETS_OK;
}

struct FpfhBatchPlan {
    std::vector<size_t> n;          // points of cluster c
    std::vector<size_t> small_n;    // n[c] on the batch route, 0 for a cluster on the work handle
    std::vector<uint32_t> src;      // n_clusters + 1: offsets[c] - offsets[0], where cluster c starts among the caller's records
    std::vector<uint32_t> bases;    // n_clusters + 1: where it starts in the concatenation (the last entry: its points)
    std::vector<RiftBatchItem> items;
    size_t n_brute = 0, n_large = 0;  // points on either route
    bool on_work_handle(size_t c) const { return n[c] != small_n[c]; }
};

// offsets[n_clusters + 1]: checked by fpfh_batch_check_offsets
inline FpfhBatchPlan fpfh_batch_plan(const size_t* offsets, size_t n_clusters, size_t limit) {
    FpfhBatchPlan p;
    p.n.assign(n_clusters, 0);
    p.small_n.assign(n_clusters, 0);
    p.src.assign(n_clusters + 1, 0u);
    for (size_t c = 0; c < n_clusters; ++c) {
        const size_t n = offsets[c + 1] - offsets[c];
        p.n[c] = n;
        p.src[c] = (uint32_t)(offsets[c] - offsets[0]);
        if (n > limit) {
            p.n_large += n;
        } else {
            p.n_brute += n;
            p.small_n[c] = n;
        }
    }
    p.src[n_clusters] = (uint32_t)(offsets[n_clusters] - offsets[0]);
    rift_batch_plan(p.small_n.data(), n_clusters, &p.bases, &p.items);
    return p;
}

// one copy of the output splice: `count` rows from row `src` of the batch route's rows to row `dst` of the caller's
struct FpfhBatchCopy {
    size_t src, dst, count;
};
// slice[n_clusters + 1]: the batch route's slice bounds (a cluster off that route owns none); single_m[c]: the rows the work
// handle found for a cluster on it.  offsets: the caller's n_clusters + 1 bounds; copies: the batch route's runs in cluster
// order, merged where neighbours stay neighbours.
template <class Slice>
inline void fpfh_batch_splice(const FpfhBatchPlan& p, const Slice* slice, const size_t* single_m, std::vector<size_t>* offsets,
                              std::vector<FpfhBatchCopy>* copies) {
    const size_t n_clusters = p.n.size();
    offsets->assign(n_clusters + 1, 0);
    copies->clear();
    size_t at = 0;
    for (size_t c = 0; c < n_clusters; ++c) {
        (*offsets)[c] = at;
        if (p.on_work_handle(c)) {
            at += single_m[c];
            continue;
        }
        const size_t src = (size_t)slice[c], m = (size_t)slice[c + 1] - src;
        if (m) {
            if (!copies->empty() && copies->back().src + copies->back().count == src && copies->back().dst + copies->back().count == at)
                copies->back().count += m;
            else
                copies->push_back({src, at, m});
        }
        at += m;
    }
    (*offsets)[n_clusters] = at;
}

}  // namespace pcc
