// rgb_merge.hpp -- the host half of pcc_region_growing_rgb (region_rgb.hip): what pcl::RegionGrowingRGB does once the
// segments are grown -- findSegmentNeighbours' cut to the nearest segments and applyRegionMergingAlgorithm -- over the
// per-segment records and the segment pair list the device hands back.  Host only, no HIP include: taken statement for
// statement from include/pcc/region_growing_rgb.hpp (findSegmentNeighbours from the heap on, mergeRegions), so that the two
// keep the same bits; tests/cpp/test_rgb_merge.cpp holds it against the oracle's restatement.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <limits>
#include <queue>
#include <utility>
#include <vector>

namespace pcc {

// one grown segment: its number of points and its channel sums (unsigned, wrapping as PCL's std::vector<unsigned int>)
struct RgbSegment {
    uint32_t size, sum_r, sum_g, sum_b;
};
// the smallest row distance from a point of segment s to a point of segment t != s (over all K row entries)
struct RgbSegmentPair {
    uint32_t s, t;
    float d2;
};

namespace rgb_merge_detail {
inline bool lessFirst(const std::pair<float, int>& a, const std::pair<float, int>& b) { return a.first < b.first; }
}  // namespace rgb_merge_detail

// segs[ns] in segment order (ascending seed index); pairs[np]: every ordered pair (s, t) at most once, in ANY order (sorted
// here, in place).  distance_threshold / region_colour_threshold are the SQUARED thresholds.  cluster_of_segment[ns] receives
// the index of the segment's cluster in PCL's output order, or -1 (size outside [min_size, max_size]); returns the number of
// clusters.
inline int rgb_merge_regions(const RgbSegment* segs, size_t ns, RgbSegmentPair* pairs, size_t np, float distance_threshold,
                             float region_colour_threshold, unsigned int region_neighbour_number, int min_pts_per_cluster,
                             int max_pts_per_cluster, std::vector<int32_t>& cluster_of_segment) {
    using rgb_merge_detail::lessFirst;
    const float fmax = std::numeric_limits<float>::max();
    // ---- findSegmentNeighbours, from the per-segment minimum distances on: the region_neighbour_number nearest, handed over
    // farthest first (PCL pops a max-heap of (distance, segment))
    std::sort(pairs, pairs + np, [](const RgbSegmentPair& a, const RgbSegmentPair& b) { return a.s != b.s ? a.s < b.s : a.t < b.t; });
    std::vector<std::vector<int> > seg_nbr(ns);
    std::vector<std::vector<float> > seg_dist(ns);
    for (size_t at = 0; at < np;) {
        const size_t s = pairs[at].s;
        std::priority_queue<std::pair<float, int> > heap;
        for (; at < np && pairs[at].s == s; ++at) {  // (ascending t: the mirror's sorted `touched`)
            heap.push(std::make_pair(pairs[at].d2, (int)pairs[at].t));
            if (heap.size() > region_neighbour_number) heap.pop();
        }
        while (!heap.empty()) {
            seg_dist[s].push_back(heap.top().first);
            seg_nbr[s].push_back(heap.top().second);
            heap.pop();
        }
    }
    // ---- mergeRegions
    // mean colour per segment as PCL's applyRegionMergingAlgorithm takes it: float(sum) / float(count) truncated to an
    // unsigned integer
    std::vector<float> col(ns * 3, 0.f);
    for (size_t s = 0; s < ns; ++s) {
        const unsigned int sum[3] = {segs[s].sum_r, segs[s].sum_g, segs[s].sum_b};
        for (int a = 0; a < 3; ++a)
            col[s * 3 + a] = (float)static_cast<unsigned int>(static_cast<float>(sum[a]) / static_cast<float>((int)segs[s].size));
    }
    std::vector<int> seg_region(ns, -1);
    std::vector<unsigned int> reg_pts;
    std::vector<int> reg_segs;
    for (size_t s = 0; s < ns; ++s) {
        int cur;
        if (seg_region[s] == -1) {
            cur = (int)reg_pts.size();
            seg_region[s] = cur;
            reg_pts.push_back((unsigned int)segs[s].size);
            reg_segs.push_back(1);
        } else {
            cur = seg_region[s];
        }
        for (size_t j = 0; j < region_neighbour_number && j < seg_nbr[s].size(); ++j) {
            const int t = seg_nbr[s][j];
            if (seg_dist[s][j] > distance_threshold) continue;
            if (seg_region[(size_t)t] != -1) continue;
            float diff = 0.f;
            for (int a = 0; a < 3; ++a) {
                const float d = col[s * 3 + a] - col[(size_t)t * 3 + a];
                diff += d * d;
            }
            if (diff < region_colour_threshold) {
                seg_region[(size_t)t] = cur;
                reg_pts[(size_t)cur] += (unsigned int)segs[(size_t)t].size;
                reg_segs[(size_t)cur] += 1;
            }
        }
    }
    const size_t nr = reg_pts.size();
    std::vector<std::vector<int> > reg_members(nr);
    for (size_t s = 0; s < ns; ++s) reg_members[(size_t)seg_region[s]].push_back((int)s);
    // neighbours of every region: the neighbour entries of its segments that lead out of it, nearest first
    std::vector<std::vector<std::pair<float, int> > > reg_nbr(nr);
    for (size_t r = 0; r < nr; ++r) {
        for (int s : reg_members[r])
            for (size_t j = 0; j < seg_nbr[(size_t)s].size(); ++j) {
                if (seg_dist[(size_t)s][j] == fmax) continue;
                const int t = seg_nbr[(size_t)s][j];
                if (seg_region[(size_t)t] != (int)r) reg_nbr[r].push_back(std::make_pair(seg_dist[(size_t)s][j], t));
            }
        std::stable_sort(reg_nbr[r].begin(), reg_nbr[r].end(), lessFirst);
    }
    // regions below the minimum size fold into the region of their nearest neighbouring segment
    for (size_t r = 0; r < nr; ++r) {
        if (reg_pts[r] >= (unsigned int)min_pts_per_cluster) continue;
        if (reg_nbr[r].empty() || reg_nbr[r][0].first == fmax) continue;
        const int into = seg_region[(size_t)reg_nbr[r][0].second];
        const std::vector<int> moved = reg_members[r];
        for (int s : moved) {
            reg_members[(size_t)into].push_back(s);
            seg_region[(size_t)s] = into;
        }
        reg_members[r].clear();
        reg_pts[(size_t)into] += reg_pts[r];
        reg_pts[r] = 0;
        reg_segs[(size_t)into] += reg_segs[r];
        reg_segs[r] = 0;
        for (std::pair<float, int>& e : reg_nbr[(size_t)into])
            if (seg_region[(size_t)e.second] == into) { e.first = fmax; e.second = 0; }
        for (const std::pair<float, int>& e : reg_nbr[r])
            if (seg_region[(size_t)e.second] != into) reg_nbr[(size_t)into].push_back(e);
        reg_nbr[r].clear();
        std::stable_sort(reg_nbr[(size_t)into].begin(), reg_nbr[(size_t)into].end(), lessFirst);
    }
    // the regions as clusters: empty regions dropped, then the size filter of extract() -- a cluster's size is the number
    // of points of its segments
    std::vector<size_t> members(nr, 0);
    for (size_t s = 0; s < ns; ++s) members[(size_t)seg_region[s]] += segs[s].size;
    std::vector<int32_t> cluster_of_region(nr, -1);
    int ncl = 0;
    for (size_t r = 0; r < nr; ++r) {
        if (members[r] == 0) continue;
        if ((int)members[r] >= min_pts_per_cluster && (int)members[r] <= max_pts_per_cluster) cluster_of_region[r] = ncl++;
    }
    cluster_of_segment.assign(ns, -1);
    for (size_t s = 0; s < ns; ++s) cluster_of_segment[s] = cluster_of_region[(size_t)seg_region[s]];
    return ncl;
}

}  // namespace pcc
