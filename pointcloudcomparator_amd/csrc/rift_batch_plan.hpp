// rift_batch_plan.hpp -- the host-built table of work items of pcc_rift_descriptors_batch's row builder (rift_batch.hip).
// Plain C++ (no HIP): tests/cpp/test_rift_batch_plan.cpp compiles it on its own.
//
// The clouds of a batch are concatenated: point i of cloud c is point base[c] + i, base = the prefix sums of the sizes.  One
// work item is one workgroup's share: RB_QUERIES consecutive points of ONE cloud as queries against that cloud alone.  Every
// (cloud, point) is a query of exactly one item and no item crosses a cloud, so no row can hold a point of another cloud.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

namespace pcc {

constexpr unsigned int RB_QUERIES = 64;     // queries of a work item at most: 16 per wave of the 256-lane workgroup
constexpr unsigned int RB_QUERIES_MIN = 4;  // ... and at least: one per wave
constexpr size_t RB_ITEMS_WANTED = 1024;    // 256 CUs x the 4 workgroups of 32 KB LDS a CU holds
constexpr unsigned int RB_TILE = 2048;      // points of the cloud a workgroup holds in LDS at a time (32 KB)

// points [base, base + n) of the concatenation are the item's cloud; its queries are base + q0 .. base + q0 + nq
struct RiftBatchItem {
    uint32_t base, n, q0, nq;
};

// the query block of a batch: the largest of 64, 32, ... 4 that yields RB_ITEMS_WANTED items, else 4
inline unsigned int rift_batch_block(const size_t* n, size_t n_clouds) {
    unsigned int block = RB_QUERIES;
    for (; block > RB_QUERIES_MIN; block /= 2) {
        size_t items = 0;
        for (size_t c = 0; c < n_clouds; ++c) items += (n[c] + block - 1) / block;
        if (items >= RB_ITEMS_WANTED) break;
    }
    return block;
}

// bases: n_clouds + 1 prefix sums of n[]; items: every cloud's query blocks in cloud order (an empty cloud has none).
// Returns the block size used.  The caller has checked that sum(n) fits 31 bits.
inline unsigned int rift_batch_plan(const size_t* n, size_t n_clouds, std::vector<uint32_t>* bases, std::vector<RiftBatchItem>* items) {
    const unsigned int block = rift_batch_block(n, n_clouds);
    bases->assign(n_clouds + 1, 0u);
    items->clear();
    size_t at = 0;
    for (size_t c = 0; c < n_clouds; ++c) {
        (*bases)[c] = (uint32_t)at;
        for (size_t q0 = 0; q0 < n[c]; q0 += block) {
            const size_t left = n[c] - q0;
            items->push_back({(uint32_t)at, (uint32_t)n[c], (uint32_t)q0, (uint32_t)(left < block ? left : block)});
        }
        at += n[c];
    }
    (*bases)[n_clouds] = (uint32_t)at;
    return block;
}

}  // namespace pcc
