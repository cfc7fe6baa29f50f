// sift_batch_plan.hpp -- the host-built tables of pcc_sift_keypoints_batch (sift_batch.hip), rebuilt for every octave round.
// Plain C++ (no HIP): tests/cpp/test_sift_batch_plan.cpp compiles it on its own.
//
// The octave clouds of a round are concatenated: point i of cloud c is point base[c] + i, base = the prefix sums of the sizes
// the voxel stage of the round reported.  A cloud that is empty, or that came out of the voxel stage with fewer points than
// the detector's gate, has LEFT the batch: its size is 0 from that round on, it owns no point of the concatenation and no work
// item.  The work items are rift_batch_plan.hpp's (query blocks of one cloud each): the radius rows and the 25-NN rows of a
// round are built from the same table, so no row can hold a point of another cloud.
// After the last round the keypoints lie in (round, cloud, point, scale) order; the caller wants (cloud, round, point, scale):
// sift_batch_splice lists the copies.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "cloud_batch.hpp"

namespace pcc {

// one round's concatenation
struct SiftBatchRound {
    std::vector<size_t> n;             // points of cloud c in this round (0: it has left the batch)
    std::vector<uint32_t> bases;       // n_clouds + 1 prefix sums of n
    std::vector<int64_t> bases64;      // the same, as the CSR offsets the voxel keys are sorted by (one row per cloud)
    std::vector<RiftBatchItem> items;  // the query blocks of the clouds still in the batch, in cloud order
    size_t total = 0;                  // bases[n_clouds]
};

// sizes[c]: the points cloud c came out of the round's voxel stage with (the caller's sizes for the table in front of the first
// round, with min_points = 0: the gate is applied to octave clouds only).  Clouds below min_points leave.
template <class Size>
inline void sift_batch_round(const Size* sizes, size_t n_clouds, size_t min_points, SiftBatchRound* r) {
    r->n.assign(n_clouds, 0);
    for (size_t c = 0; c < n_clouds; ++c) r->n[c] = (size_t)sizes[c] >= min_points ? (size_t)sizes[c] : 0;
    rift_batch_plan(r->n.data(), n_clouds, &r->bases, &r->items);
    r->bases64.assign(r->bases.begin(), r->bases.end());
    r->total = r->bases[n_clouds];
}

// bases + bases64 + items of a round, laid out for one copy behind at0 bytes of the caller's
struct TableLayout {
    size_t bases_at, bases64_at, items_at, bytes;
    TableLayout(size_t n_clouds, size_t n_items, size_t at0 = 0) {
        bases64_at = align_up(at0, 16);
        bases_at = bases64_at + (n_clouds + 1) * sizeof(int64_t);
        items_at = align_up(bases_at + (n_clouds + 1) * sizeof(uint32_t), 16);
        bytes = align_up(items_at + n_items * sizeof(RiftBatchItem), 16);
    }
    void fill(char* u, const SiftBatchRound& r) const {
        memcpy(u + bases64_at, r.bases64.data(), r.bases64.size() * sizeof(int64_t));
        memcpy(u + bases_at, r.bases.data(), r.bases.size() * sizeof(uint32_t));
        if (!r.items.empty()) memcpy(u + items_at, r.items.data(), r.items.size() * sizeof(RiftBatchItem));
    }
};

// one copy of the splice: `count` keypoints from row `src` of the round-major buffer to row `dst` of the caller's array
struct SiftBatchCopy {
    size_t src, dst, count;
};

// counts[r][c]: the keypoints round r found in cloud c.  offsets: n_clouds + 1 slice bounds of the caller's array; copies: in
// (cloud, round) order, empty ones left out.
inline void sift_batch_splice(const std::vector<std::vector<uint32_t>>& counts, size_t n_clouds, std::vector<size_t>* offsets,
                              std::vector<SiftBatchCopy>* copies) {
    offsets->assign(n_clouds + 1, 0);
    copies->clear();
    std::vector<size_t> round_at(counts.size() + 1, 0), within(counts.size(), 0);
    for (size_t r = 0; r < counts.size(); ++r) {
        size_t sum = 0;
        for (size_t c = 0; c < n_clouds; ++c) sum += counts[r][c];
        round_at[r + 1] = round_at[r] + sum;
    }
    size_t at = 0;
    for (size_t c = 0; c < n_clouds; ++c) {
        (*offsets)[c] = at;
        for (size_t r = 0; r < counts.size(); ++r) {
            const size_t m = counts[r][c];
            if (m) copies->push_back({round_at[r] + within[r], at, m});
            within[r] += m;
            at += m;
        }
    }
    (*offsets)[n_clouds] = at;
}

}  // namespace pcc
