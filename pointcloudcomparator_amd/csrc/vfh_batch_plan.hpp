// vfh_batch_plan.hpp -- the host-built tables of pcc_vfh_descriptors_batch (vfh_batch.hip).
// Plain C++ (no HIP): tests/cpp/test_vfh_batch_plan.cpp compiles it on its own.
//
// The clusters of a call are ranges of ONE array of records: cluster c is records offsets[c] .. offsets[c + 1].  VFH is a global
// descriptor: a cluster of 2 points and more has exactly one, a smaller one has none -- so the caller's bounds out_offsets are
// the prefix sums of (n >= 2), known before anything is launched, and every descriptor's row in the caller's array with them.
// Three kinds of cluster:
//   2 .. limit points   the batch route: the concatenation the batch kernels run over (bases and row-builder items as
//                       rift_batch_plan builds them; a cluster off that route has size 0 there and shares its base with the
//                       cluster behind it);
//   above the limit     the single call on the work handle, one by one, straight into the cluster's row;
//   0 or 1 points       neither route: never read, no row.
// The vote items: one item is up to VFH_BATCH_VOTE_POINTS consecutive points of ONE cluster, one workgroup's share of the vote
// kernel -- its LDS table of counters belongs to one cluster.  The copy runs: for a caller in host memory the batch route's rows
// are written to a staging array laid out like the caller's and copied down run by run, a run ending where a cluster on the work
// handle owns the next row.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "fpfh_batch_plan.hpp"

namespace pcc {

// Points of a vote item at most.  A 256-lane workgroup clears and flushes a table of 263 counters per item: at 1024 points that
// is at most one global atomic per four points and four points a lane, while a comparison's clusters (60 to 200 of 300 to 5000
// points) still give one to five items each -- as many workgroups as the chip has CUs.  The votes are a few per cent of a call
// (the chains bound it): nothing smaller was worth measuring.
constexpr unsigned int VFH_BATCH_VOTE_POINTS = 1024;
constexpr size_t VFH_MIN_POINTS = 2;  // PCL's initCompute fails below: no descriptor

// points [first, first + count) of the concatenation, all of cluster `cluster`
struct VfhVoteItem {
    uint32_t cluster, first, count, pad;
};
// rows [row, row + count) of the staging array go to the same rows of the caller's
struct VfhBatchCopy {
    size_t row, count;
};

struct VfhBatchPlan {
    std::vector<size_t> n;          // points of cluster c
    std::vector<size_t> small_n;    // n[c] on the batch route, else 0
    std::vector<uint32_t> src;      // n_clusters + 1: offsets[c] - offsets[0], where cluster c starts among the caller's records
    std::vector<uint32_t> bases;    // n_clusters + 1: where it starts in the concatenation (the last entry: its points)
    std::vector<RiftBatchItem> items;   // the row builder's work items
    std::vector<VfhVoteItem> votes;     // the vote kernel's
    std::vector<uint32_t> route;        // the clusters on the batch route, ascending: one chain workgroup and one finish workgroup each
    std::vector<uint32_t> row;          // n_clusters: out_offsets[c] in 32 bits, the cluster's row in the caller's array
    std::vector<size_t> out_offsets;    // n_clusters + 1: the caller's bounds
    std::vector<VfhBatchCopy> copies;   // the batch route's rows in cluster order, merged where neighbours stay neighbours
    size_t n_brute = 0, n_large = 0;    // points on either route
    bool on_batch_route(size_t c) const { return small_n[c] != 0; }
    bool on_work_handle(size_t c) const { return n[c] >= VFH_MIN_POINTS && small_n[c] == 0; }
    size_t descriptors() const { return out_offsets.back(); }
};

// offsets[n_clusters + 1]: checked by fpfh_batch_check_offsets
inline VfhBatchPlan vfh_batch_plan(const size_t* offsets, size_t n_clusters, size_t limit) {
    VfhBatchPlan p;
    p.n.assign(n_clusters, 0);
    p.small_n.assign(n_clusters, 0);
    p.src.assign(n_clusters + 1, 0u);
    p.row.assign(n_clusters, 0u);
    p.out_offsets.assign(n_clusters + 1, 0);
    size_t rows = 0;
    for (size_t c = 0; c < n_clusters; ++c) {
        const size_t n = offsets[c + 1] - offsets[c];
        p.n[c] = n;
        p.src[c] = (uint32_t)(offsets[c] - offsets[0]);
        p.out_offsets[c] = rows;
        p.row[c] = (uint32_t)rows;
        if (n < VFH_MIN_POINTS) continue;
        if (n > limit) {
            p.n_large += n;
        } else {
            p.n_brute += n;
            p.small_n[c] = n;
            p.route.push_back((uint32_t)c);
            if (!p.copies.empty() && p.copies.back().row + p.copies.back().count == rows) ++p.copies.back().count;
            else p.copies.push_back({rows, 1});
        }
        ++rows;
    }
    p.src[n_clusters] = n_clusters ? (uint32_t)(offsets[n_clusters] - offsets[0]) : 0u;
    p.out_offsets[n_clusters] = rows;
    rift_batch_plan(p.small_n.data(), n_clusters, &p.bases, &p.items);
    for (const uint32_t c : p.route)
        for (size_t i0 = 0; i0 < p.small_n[c]; i0 += VFH_BATCH_VOTE_POINTS) {
            const size_t left = p.small_n[c] - i0;
            p.votes.push_back({c, p.bases[c] + (uint32_t)i0, (uint32_t)(left < VFH_BATCH_VOTE_POINTS ? left : VFH_BATCH_VOTE_POINTS), 0u});
        }
    return p;
}

}  // namespace pcc
