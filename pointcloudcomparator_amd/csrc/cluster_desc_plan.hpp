// cluster_desc_plan.hpp -- the host-built tables of pcc_cluster_descriptors (cluster_desc.hip).
// Plain C++ (no HIP): tests/cpp/test_cluster_desc_plan.cpp compiles it on its own.
//
// The clusters of a call are staged ONCE as 32-byte records: the clusters of the SIFT batch route first, in cluster order -- that
// prefix is the first concatenation of the octave rounds, whose table gives every other cluster size 0 --, the others behind it
// in cluster order.  The keypoints of the rounds lie round-major on the device, those of the clusters sent through the work
// handle behind them, cluster by cluster; cd_keypoint_order lists them cluster-major.  Once the snapped points of every cluster
// are counted, every cluster has a cloud for RIFT (its own points on the dense route, its snapped points on the SIFT route): the
// clouds up to the limit form the RIFT concatenation, the larger ones lie behind it and take the single path.  cd_splice puts
// the slices of both back into cluster order.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "rift_batch_plan.hpp"

namespace pcc {

enum : uint32_t { CD_DENSE = 0, CD_SIFT_BATCH = 1, CD_SIFT_WORK = 2 };

struct ClusterDescRoutes {
    std::vector<uint32_t> route;       // CD_* of cluster c
    std::vector<size_t> n;             // points of cluster c
    std::vector<size_t> sift_n;        // n[c] on the SIFT batch route, else 0: the sizes of the rounds' first table
    std::vector<uint32_t> stage_base;  // n_clusters + 1: cluster c's records start here (the last entry: all staged points)
    size_t n_dense = 0, n_sift = 0;    // points on either route
    size_t sift_batch_total = 0;       // points of the rounds' first concatenation (the staged prefix)
};

// offsets[n_clusters + 1], non-decreasing, fewer than 2^31 points (the caller has checked both)
inline ClusterDescRoutes cd_routes(const size_t* offsets, size_t n_clusters, size_t sift_above, size_t sift_batch_max) {
    ClusterDescRoutes r;
    r.route.assign(n_clusters, CD_DENSE);
    r.n.assign(n_clusters, 0);
    r.sift_n.assign(n_clusters, 0);
    r.stage_base.assign(n_clusters + 1, 0);
    size_t at = 0;
    for (size_t c = 0; c < n_clusters; ++c) {
        const size_t n = offsets[c + 1] - offsets[c];
        r.n[c] = n;
        if (n > sift_above) {
            r.n_sift += n;
            r.route[c] = n > sift_batch_max ? CD_SIFT_WORK : CD_SIFT_BATCH;
        } else {
            r.n_dense += n;
        }
        if (r.route[c] == CD_SIFT_BATCH) {
            r.sift_n[c] = n;
            r.stage_base[c] = (uint32_t)at;
            at += n;
        }
    }
    r.sift_batch_total = at;
    for (size_t c = 0; c < n_clusters; ++c) {
        if (r.route[c] == CD_SIFT_BATCH) continue;
        r.stage_base[c] = (uint32_t)at;
        at += r.n[c];
    }
    r.stage_base[n_clusters] = (uint32_t)at;
    return r;
}

// counts[r][c]: the keypoints round r found in cluster c (round-major on the device: round 0's in cluster order, then round
// 1's ...); work_counts[c]: the keypoints of a cluster sent through the work handle, which lie behind all of those, cluster
// by cluster.  kbase: n_clusters + 1 prefix sums of the keypoints per cluster; order[k]: where keypoint k of the
// (cluster, round, point, scale) order lies on the device.
inline void cd_keypoint_order(const std::vector<std::vector<uint32_t>>& counts, const std::vector<uint32_t>& work_counts, size_t n_clusters,
                              std::vector<uint32_t>* kbase, std::vector<uint32_t>* order) {
    kbase->assign(n_clusters + 1, 0u);
    order->clear();
    std::vector<size_t> round_at(counts.size() + 1, 0), within(counts.size(), 0);
    for (size_t r = 0; r < counts.size(); ++r) {
        size_t sum = 0;
        for (size_t c = 0; c < n_clusters; ++c) sum += counts[r][c];
        round_at[r + 1] = round_at[r] + sum;
    }
    size_t work_at = round_at[counts.size()];
    for (size_t c = 0; c < n_clusters; ++c) {
        (*kbase)[c] = (uint32_t)order->size();
        for (size_t r = 0; r < counts.size(); ++r) {
            for (uint32_t i = 0; i < counts[r][c]; ++i) order->push_back((uint32_t)(round_at[r] + within[r] + i));
            within[r] += counts[r][c];
        }
        const uint32_t w = c < work_counts.size() ? work_counts[c] : 0u;
        for (uint32_t i = 0; i < w; ++i) order->push_back((uint32_t)(work_at + i));
        work_at += w;
    }
    (*kbase)[n_clusters] = (uint32_t)order->size();
}

// The clouds RIFT runs over: q_n[c] points each.  Those up to rift_batch_max form the concatenation (small_n, bases and items
// as rift_batch_plan builds them); the others lie behind it.  dst[c]: where cloud c starts; dst[n_clusters]: all points.
struct ClusterDescClouds {
    std::vector<size_t> small_n;
    std::vector<uint32_t> bases, dst;
    std::vector<RiftBatchItem> items;
    size_t n_batch = 0, n_single = 0;  // points on either route
};
inline ClusterDescClouds cd_clouds(const size_t* q_n, size_t n_clusters, size_t rift_batch_max) {
    ClusterDescClouds p;
    p.small_n.assign(q_n, q_n + n_clusters);
    for (size_t c = 0; c < n_clusters; ++c) {
        (q_n[c] > rift_batch_max ? p.n_single : p.n_batch) += q_n[c];
        if (q_n[c] > rift_batch_max) p.small_n[c] = 0;
    }
    rift_batch_plan(p.small_n.data(), n_clusters, &p.bases, &p.items);
    p.dst.assign(p.bases.begin(), p.bases.end());
    size_t at = p.bases[n_clusters];
    for (size_t c = 0; c < n_clusters; ++c) {
        if (q_n[c] <= rift_batch_max) continue;
        p.dst[c] = (uint32_t)at;
        at += q_n[c];
    }
    p.dst[n_clusters] = (uint32_t)at;
    return p;
}

// one copy of the output splice: `count` descriptors from row `src` of the batch route's rows to row `dst` of the caller's
struct ClusterDescCopy {
    size_t src, dst, count;
};
// slice[n_clusters + 1]: the batch route's slice bounds (a cloud off that route owns none); single_m[c]: the descriptors the
// single path found for a cloud off it.  offsets: the caller's n_clusters + 1 bounds; copies: the batch route's runs, merged
// where neighbours stay neighbours.
template <class Slice>
inline void cd_splice(const Slice* slice, const size_t* q_n, const size_t* single_m, size_t n_clusters, size_t rift_batch_max,
                      std::vector<size_t>* offsets, std::vector<ClusterDescCopy>* copies) {
    offsets->assign(n_clusters + 1, 0);
    copies->clear();
    size_t at = 0;
    for (size_t c = 0; c < n_clusters; ++c) {
        (*offsets)[c] = at;
        if (q_n[c] > rift_batch_max) {
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
