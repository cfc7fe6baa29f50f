// match_colour_plan.hpp -- the host decisions of pcc_match_colour_elements (match_colour.hip): which clusters of the two scenes the
// match table names, each ONCE, and where each goes.  Plain C++ (no HIP): tests/cpp/test_match_colour_plan.cpp compiles it on
// its own.
//
// The reference's match loop (src/comparator.cpp:1379-1509) runs color_growing_segmentation on both clusters of every accepted
// match and keeps the two segment counts.  closestCentroid's exclusion set is per cluster of scene 1, so several clusters of
// scene 1 can be matched to the same cluster of scene 2: the distinct (scene, cluster) pairs are listed here in first-use order
// -- (i, scene 1) before (i, scene 2), i ascending -- and every (i, side) of the table maps back to its entry of that list.  A
// cluster of up to `brute_limit` records joins the concatenation of the batch route (its clouds in list order, bases = the
// prefix sums of their sizes, query blocks from rift_batch_plan.hpp); a larger one goes through the work handle on its own.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "rift_batch_plan.hpp"

namespace pcc {

enum { MC_BATCH = 0, MC_WORK = 1 };

// a distinct cluster the match table names: records src0 .. src0 + n of its scene's arrays
struct MatchColourCluster {
    uint32_t scene;    // 0: scene 1, 1: scene 2
    uint32_t cluster;  // its index in the scene
    uint32_t route;    // MC_BATCH or MC_WORK
    uint32_t slot;     // MC_BATCH: its cloud of the concatenation; MC_WORK: its place among the clusters of the work handle
    uint64_t src0;
    uint32_t n;
    uint32_t base;     // MC_BATCH: its first point of the concatenation (= bases[slot]); MC_WORK: 0
};

struct MatchColourPlan {
    std::vector<MatchColourCluster> clusters;  // first-use order
    std::vector<int32_t> entry;                // [n_clusters1][2]: the place of (i, side) in `clusters`, -1 without a match
    std::vector<size_t> batch_n;               // the sizes of the concatenation's clouds, in slot order
    std::vector<uint32_t> bases;               // batch_n.size() + 1 prefix sums of batch_n
    std::vector<RiftBatchItem> items;          // rift_batch_plan's query blocks over batch_n
    size_t n_batch_points = 0, n_work_points = 0;  // records on either route
    size_t n_work = 0;                             // clusters on the work route
    size_t n_saved = 0;                            // (i, side) entries that name a cluster listed before
};

// matches[i] in [-1, n_clusters2) and non-decreasing offsets spanning fewer than 2^31 records are the caller's to have checked.
// false -- nothing usable in *plan -- when the batch route would hold 2^31 points and more.
inline bool mc_plan(const int32_t* matches, size_t n_clusters1, const size_t* offsets1, size_t n_clusters2, const size_t* offsets2,
                    size_t brute_limit, MatchColourPlan* plan) {
    MatchColourPlan& P = *plan;
    P = MatchColourPlan();
    P.entry.assign(2 * n_clusters1, -1);
    std::vector<int32_t> seen2(n_clusters2, -1);  // (a cluster of scene 1 is named by its own row alone)
    for (size_t i = 0; i < n_clusters1; ++i) {
        if (matches[i] < 0) continue;
        for (uint32_t side = 0; side < 2; ++side) {
            const size_t c = side ? (size_t)matches[i] : i;
            if (side && seen2[c] >= 0) {
                P.entry[2 * i + 1] = seen2[c];
                ++P.n_saved;
                continue;
            }
            const size_t* off = side ? offsets2 : offsets1;
            MatchColourCluster m;
            m.scene = side;
            m.cluster = (uint32_t)c;
            m.src0 = off[c];
            m.n = (uint32_t)(off[c + 1] - off[c]);
            m.route = m.n > brute_limit ? MC_WORK : MC_BATCH;
            m.base = 0;
            if (m.route == MC_BATCH) {
                m.slot = (uint32_t)P.batch_n.size();
                m.base = (uint32_t)P.n_batch_points;
                P.batch_n.push_back(m.n);
                P.n_batch_points += m.n;
                if (P.n_batch_points >= ((size_t)1 << 31)) return false;
            } else {
                m.slot = (uint32_t)P.n_work++;
                P.n_work_points += m.n;
            }
            P.entry[2 * i + side] = (int32_t)P.clusters.size();
            if (side) seen2[c] = (int32_t)P.clusters.size();
            P.clusters.push_back(m);
        }
    }
    rift_batch_plan(P.batch_n.data(), P.batch_n.size(), &P.bases, &P.items);
    return true;
}

// out_elements[i] = {-1, -1} without a match, else the counts of the two entries (i, side) maps to
inline void mc_fill(const MatchColourPlan& P, const int32_t* count_of_cluster, size_t n_clusters1, int32_t* out_elements) {
    for (size_t e = 0; e < 2 * n_clusters1; ++e) out_elements[e] = P.entry[e] < 0 ? -1 : count_of_cluster[P.entry[e]];
}

}  // namespace pcc
