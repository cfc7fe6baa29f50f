// cluster_match_plan.hpp -- the host side of pcc_cluster_matching (cluster_match.hip): the decisions of the reference's
// cluster-matching loop (src/comparator.cpp:1296-1366; pointcloudcomparator_amd/host/report.hpp: clusterSections,
// nearestFreeCentroid) and the tables of the one search behind it.  Plain C++ (no HIP): tests/cpp/test_cluster_match_plan.cpp
// compiles it on its own.
//
// The loop, per cluster i of scene 1: the three nearest free centroids of scene 2 (cm_candidates), two gates in front of
// matchRIFTFeaturesKnn (cm_states), the search of every pair that passed them -- of which the loop reads the NUMBER of
// correspondences only --, and the integer-division acceptance rule (cm_accept).  Everything but the search is
// O(n_clusters1 * n_clusters2) on a few hundred clusters and stays here; its double pow / float sqrt are the host's own.
//
// The search tables (cm_layout): every cluster of either scene that takes part in a searched pair is packed ONCE, as
// match_dims_plan.hpp's record (DP floats, zero padding, an invalid record as (+inf, 0, ...)) -- a scene-2 cluster is typically a
// candidate of several scene-1 clusters, and pcc_match_knn_batch packs it once per pair.  The table of work items and its slice
// are match_plan.hpp's: a pair's queries are its scene-2 records, its references its scene-1 records.  A (pair, query) owns one
// result slot: the bits of its smallest distance.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <cmath>
#include <vector>

#include "match_dims_plan.hpp"

namespace pcc {

enum { CM_NONE = 0, CM_GATED_COUNTS = 1, CM_GATED_SIZE = 2, CM_SEARCHED = 3 };

// nearestFreeCentroid (reference :1069-1087) with the taken set as two indices (-1: none): differences in float, squares and
// their sum in double, the sum rounded to float, a float square root, strict < against a start value of 1e12f.  -1 when nothing
// qualifies (no free centroid, NaN, a distance of 1e12 or more); among equal distances the lowest index.
inline int32_t cm_nearest_free(const float c[3], const float* centroids, size_t n, int32_t taken0, int32_t taken1) {
    int32_t arg = -1;
    float best = 1000000000000.f;
    for (size_t j = 0; j < n; ++j) {
        if ((int32_t)j == taken0 || (int32_t)j == taken1) continue;
        const float* o = centroids + 3 * j;
        const float d2 = std::pow(c[0] - o[0], 2) + std::pow(c[1] - o[1], 2) + std::pow(c[2] - o[2], 2);
        const float d = std::sqrt(d2);
        if (d < best) { best = d; arg = (int32_t)j; }
    }
    return arg;
}

// candidates[i][k], k = 0, 1, 2: cm_nearest_free applied three times, results 0 and 1 joining the taken set
inline void cm_candidates(const float* centroids1, size_t n_clusters1, const float* centroids2, size_t n_clusters2, int32_t* candidates) {
    for (size_t i = 0; i < n_clusters1; ++i) {
        int32_t* c = candidates + 3 * i;
        c[0] = cm_nearest_free(centroids1 + 3 * i, centroids2, n_clusters2, -1, -1);
        c[1] = cm_nearest_free(centroids1 + 3 * i, centroids2, n_clusters2, c[0], -1);
        c[2] = cm_nearest_free(centroids1 + 3 * i, centroids2, n_clusters2, c[0], c[1]);
    }
}

// state[i][k]: CM_NONE without a candidate; CM_GATED_COUNTS unless both descriptor counts exceed 3 (evaluated first);
// CM_GATED_SIZE unless points2[j] / points1[i] == 1 as size_t division (points1[i] == 0: gated out, not divided by);
// CM_SEARCHED otherwise.  offsets_s[c + 1] - offsets_s[c] is the descriptor count of cluster c of scene s.
inline void cm_states(const int32_t* candidates, size_t n_clusters1, const size_t* offsets1, const size_t* offsets2, const size_t* points1,
                      const size_t* points2, int32_t* state) {
    for (size_t i = 0; i < n_clusters1; ++i) {
        const size_t n1 = offsets1[i + 1] - offsets1[i];
        for (int k = 0; k < 3; ++k) {
            const int32_t j = candidates[3 * i + k];
            int32_t& s = state[3 * i + k];
            if (j < 0) { s = CM_NONE; continue; }
            const size_t n2 = offsets2[j + 1] - offsets2[j];
            if (n1 <= 3 || n2 <= 3) { s = CM_GATED_COUNTS; continue; }
            if (points1[i] == 0 || points2[j] / points1[i] != 1) { s = CM_GATED_SIZE; continue; }
            s = CM_SEARCHED;
        }
    }
}

// matches[i]: -1 and best = 0 to start with; for k = 0, 1, 2 in state CM_SEARCHED, corr = correspondences[i][k] and denom = the
// larger descriptor count: accepted when corr / denom >= 1 (integer division) and corr > best; then best = corr, matches[i] = j
inline void cm_accept(const int32_t* candidates, const int32_t* state, const uint32_t* correspondences, size_t n_clusters1,
                      const size_t* offsets1, const size_t* offsets2, int32_t* matches) {
    for (size_t i = 0; i < n_clusters1; ++i) {
        matches[i] = -1;
        size_t best = 0;
        const size_t n1 = offsets1[i + 1] - offsets1[i];
        for (int k = 0; k < 3; ++k) {
            if (state[3 * i + k] != CM_SEARCHED) continue;
            const int32_t j = candidates[3 * i + k];
            const size_t n2 = offsets2[j + 1] - offsets2[j];
            const size_t corr = correspondences[3 * i + k], denom = n1 > n2 ? n1 : n2;
            if (corr / denom >= 1 && corr > best) { best = corr; matches[i] = j; }
        }
    }
}

// a searched pair: its nq result slots from slot0, its count to out[out] (out = 3 * i + k)
struct ClusterMatchPair {
    uint32_t slot0, nq, out, pad;
};
// a packed cluster: records src0 .. src0 + n of the scene's descriptor array (side 0: des1, 1: des2) at rec0 ... of the packed ones
struct ClusterMatchCloud {
    uint32_t rec0, n, side, pad;
    uint64_t src0;
};

struct ClusterMatchLayout {
    std::vector<ClusterMatchCloud> clouds;  // scene 1's clusters that take part, in cluster order, then scene 2's
    std::vector<ClusterMatchPair> pairs;    // in (i, k) order
    std::vector<MatchItem> items;           // (match_plan.hpp; the minimum of query q0 + i goes to slot qslot0 + i)
    size_t n_rec = 0, n_slots = 0;          // packed records; result slots (= queries over all searched pairs)
    unsigned int slice = 0;                 // references per item at most
};

// Lays out the packed records and builds the pair and item tables of the pairs in state CM_SEARCHED.
// false: 2^31 records, slots or items and more (nothing usable in *layout).
inline bool cm_layout(const int32_t* candidates, const int32_t* state, size_t n_clusters1, size_t n_clusters2, const size_t* offsets1,
                      const size_t* offsets2, int dp, ClusterMatchLayout* layout) {
    ClusterMatchLayout& L = *layout;
    L.clouds.clear();
    L.pairs.clear();
    L.items.clear();
    L.n_rec = L.n_slots = 0;
    L.slice = 0;
    std::vector<char> used1(n_clusters1, 0), used2(n_clusters2, 0);
    for (size_t e = 0; e < 3 * n_clusters1; ++e)
        if (state[e] == CM_SEARCHED) { used1[e / 3] = 1; used2[(size_t)candidates[e]] = 1; }
    std::vector<size_t> rec1(n_clusters1, 0), rec2(n_clusters2, 0);
    for (int side = 0; side < 2; ++side) {
        const size_t nc = side ? n_clusters2 : n_clusters1;
        const size_t* off = side ? offsets2 : offsets1;
        for (size_t c = 0; c < nc; ++c) {
            if (!(side ? used2[c] : used1[c])) continue;
            const size_t n = off[c + 1] - off[c];
            (side ? rec2 : rec1)[c] = L.n_rec;
            if (L.n_rec + n >= MATCH_LIMIT) return false;
            L.clouds.push_back({(uint32_t)L.n_rec, (uint32_t)n, (uint32_t)side, 0u, (uint64_t)off[c]});
            L.n_rec += n;
        }
    }
    std::vector<MatchPair> ps;  // scene 2's records are the queries, scene 1's the references
    for (size_t e = 0; e < 3 * n_clusters1; ++e) {
        if (state[e] != CM_SEARCHED) continue;
        const size_t i = e / 3, j = (size_t)candidates[e];
        const size_t n2 = offsets2[j + 1] - offsets2[j];
        if (L.n_slots + n2 >= MATCH_LIMIT) return false;
        L.pairs.push_back({(uint32_t)L.n_slots, (uint32_t)n2, (uint32_t)e, 0u});
        ps.push_back({rec2[j], n2, rec1[i], offsets1[i + 1] - offsets1[i], L.n_slots});
        L.n_slots += n2;
    }
    L.slice = match_slice(ps, match_dims_slice_max(dp));
    return match_items(ps, L.slice, &L.items);
}

}  // namespace pcc
