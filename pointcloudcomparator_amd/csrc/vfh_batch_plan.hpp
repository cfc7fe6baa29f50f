// vfh_batch_plan.hpp -- the host-built tables of pcc_vfh_descriptors_batch (vfh_batch.hip).
// Plain C++ (no HIP): tests/cpp/test_vfh_batch_plan.cpp compiles it on its own.
//
// The clusters of a call are ranges of ONE array of records: cluster c is records offsets[c] .. offsets[c + 1].  VFH is a global
// descriptor: a cluster of 2 points and more has exactly one, a smaller one has none -- so the caller's bounds out_offsets are
// the prefix sums of (n >= 2), known before anything is launched, and every descriptor's row in the caller's array with them.
// Three kinds of cluster (range_batch_plan.hpp: range_batch_plan with min_points = 2):
//   2 .. limit points   the batch route: the concatenation the batch kernels run over;
//   above the limit     the single call on the work handle, one by one, straight into the cluster's row;
//   0 or 1 points       neither route: never read, no row.
// The vote items: one item is up to VFH_BATCH_VOTE_POINTS consecutive points of ONE cluster, one workgroup's share of the vote
// kernel -- its LDS table of counters belongs to one cluster.  The copy runs: for a caller in host memory the batch route's rows
// are written to a staging array laid out like the caller's and copied down run by run, a run ending where a cluster on the work
// handle owns the next row.
#pragma once
#include "range_batch_plan.hpp"

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

// sizes, routes (min_points = VFH_MIN_POINTS), src, bases and row-builder items: the RangeBatchPlan; the rest is VFH's
struct VfhBatchPlan : RangeBatchPlan {
    std::vector<VfhVoteItem> votes;     // the vote kernel's
    std::vector<uint32_t> route;        // the clusters on the batch route, ascending: one chain workgroup and one finish workgroup each
    std::vector<uint32_t> row;          // n_clusters: out_offsets[c] in 32 bits, the cluster's row in the caller's array
    std::vector<size_t> out_offsets;    // n_clusters + 1: the caller's bounds
    std::vector<VfhBatchCopy> copies;   // the batch route's rows in cluster order, merged where neighbours stay neighbours
    bool on_batch_route(size_t c) const { return small_n[c] != 0; }
    size_t descriptors() const { return out_offsets.back(); }
};

// The call's own part of the upload (range_batch_plan.hpp: RangeUpload), offsets from its start `extra_at` (4-byte aligned):
// row[n_clusters] | route | the vote items at the next 16-byte boundary of the upload.
struct VfhUploadExtra {
    size_t route_at, votes_at, bytes;
    VfhUploadExtra(const VfhBatchPlan& p, size_t extra_at) {
        route_at = p.row.size() * sizeof(uint32_t);
        votes_at = align_up(extra_at + route_at + p.route.size() * sizeof(uint32_t), 16) - extra_at;
        bytes = votes_at + p.votes.size() * sizeof(VfhVoteItem);
    }
    template <class C> auto row(C* e) const { return carve<uint32_t>(e, 0); }
    template <class C> auto route(C* e) const { return carve<uint32_t>(e, route_at); }
    template <class C> auto votes(C* e) const { return carve<VfhVoteItem>(e, votes_at); }
    // (a plan with a batch route: no table is empty; the padding in front of the vote items was zeroed by RangeUpload::fill)
    void fill(char* e, const VfhBatchPlan& p) const {
        memcpy(row(e), p.row.data(), p.row.size() * sizeof(uint32_t));
        memcpy(route(e), p.route.data(), p.route.size() * sizeof(uint32_t));
        memcpy(votes(e), p.votes.data(), p.votes.size() * sizeof(VfhVoteItem));
    }
};

// offsets[n_clusters + 1]: checked by check_range_offsets
inline VfhBatchPlan vfh_batch_plan(const size_t* offsets, size_t n_clusters, size_t limit) {
    VfhBatchPlan p;
    static_cast<RangeBatchPlan&>(p) = range_batch_plan(offsets, n_clusters, VFH_MIN_POINTS, limit);
    p.row.assign(n_clusters, 0u);
    p.out_offsets.assign(n_clusters + 1, 0);
    size_t rows = 0;
    for (size_t c = 0; c < n_clusters; ++c) {
        p.out_offsets[c] = rows;
        p.row[c] = (uint32_t)rows;
        if (p.n[c] < VFH_MIN_POINTS) continue;
        if (p.on_batch_route(c)) {
            p.route.push_back((uint32_t)c);
            if (!p.copies.empty() && p.copies.back().row + p.copies.back().count == rows) ++p.copies.back().count;
            else p.copies.push_back({rows, 1});
        }
        ++rows;
    }
    p.out_offsets[n_clusters] = rows;
    for (const uint32_t c : p.route)
        for (size_t i0 = 0; i0 < p.small_n[c]; i0 += VFH_BATCH_VOTE_POINTS) {
            const size_t left = p.small_n[c] - i0;
            p.votes.push_back({c, p.bases[c] + (uint32_t)i0, (uint32_t)(left < VFH_BATCH_VOTE_POINTS ? left : VFH_BATCH_VOTE_POINTS), 0u});
        }
    return p;
}

}  // namespace pcc
