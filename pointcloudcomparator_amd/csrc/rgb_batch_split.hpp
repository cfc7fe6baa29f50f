// rgb_batch_split.hpp -- the host half of pcc_region_growing_rgb_batch (region_rgb_batch.hip): the per-segment records and the
// segment pair list of a CONCATENATION of clouds, cut per cloud and handed to rgb_merge_regions (rgb_merge.hpp) one cloud at a
// time.  Host only, no HIP include: tests/cpp/test_rgb_batch_split.cpp compiles it on its own.
//
// Segment ids are dense over the concatenation in index order, so cloud c owns the ids id_base[c] .. id_base[c + 1] (a cloud
// without a finite point owns none).  The pair list is sorted ONCE by (s, t); the pairs of a cloud are then one run of it, and
// both ends of every pair of the run lie in the cloud's id range -- rows never cross a cloud.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

#include "rgb_merge.hpp"

namespace pcc {

// segs[ns], pairs[np] (any order; sorted here, in place), id_base[n_clouds + 1] ascending with id_base[n_clouds] == ns; the
// thresholds are the SQUARED ones, as rgb_merge_regions takes them.  cluster_of_segment[ns]: the cluster of every segment
// LOCAL to its cloud (PCL's output order there) or -1; n_clusters[n_clouds].  Returns false -- nothing usable written -- when
// the id ranges do not tile [0, ns) or a pair leaves its cloud.
inline bool rgb_batch_split(const RgbSegment* segs, size_t ns, RgbSegmentPair* pairs, size_t np, const uint32_t* id_base, size_t n_clouds,
                            float distance_threshold, float region_colour_threshold, unsigned int region_neighbour_number,
                            int min_pts_per_cluster, int max_pts_per_cluster, std::vector<int32_t>& cluster_of_segment,
                            int32_t* n_clusters) {
    if (n_clouds == 0 ? ns != 0 : (id_base[0] != 0 || id_base[n_clouds] != ns)) return false;
    std::sort(pairs, pairs + np, [](const RgbSegmentPair& a, const RgbSegmentPair& b) { return a.s != b.s ? a.s < b.s : a.t < b.t; });
    cluster_of_segment.assign(ns, -1);
    std::vector<RgbSegmentPair> local;
    std::vector<int32_t> of_segment;
    size_t at = 0;
    for (size_t c = 0; c < n_clouds; ++c) {
        const uint32_t lo = id_base[c], hi = id_base[c + 1];
        if (hi < lo || hi > ns) return false;
        local.clear();
        for (; at < np && pairs[at].s < hi; ++at) {
            const RgbSegmentPair& p = pairs[at];
            if (p.s < lo || p.t < lo || p.t >= hi) return false;  // a pair between two clouds
            local.push_back(RgbSegmentPair{p.s - lo, p.t - lo, p.d2});
        }
        n_clusters[c] = (int32_t)rgb_merge_regions(segs + lo, (size_t)(hi - lo), local.data(), local.size(), distance_threshold,
                                                   region_colour_threshold, region_neighbour_number, min_pts_per_cluster,
                                                   max_pts_per_cluster, of_segment);
        std::copy(of_segment.begin(), of_segment.end(), cluster_of_segment.begin() + lo);
    }
    return at == np;
}

}  // namespace pcc
