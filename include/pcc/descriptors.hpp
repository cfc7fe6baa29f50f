// descriptors.hpp -- pcc::clusterDescriptors: the reference's per-cluster descriptor loop (src/comparator.cpp:1224-1290) in ONE
// library call (pcc_cluster_descriptors).  A cluster above `sift_above` points (700 in the reference, :1228-1231, :1264-1265)
// gets what pcc::processRIFTwithSIFT returns for it, the others what pcc::processRIFT returns; every cluster's centroid
// (:1235-1247) comes with them.  Neither keypoints nor snapped clouds visit the host in between.
// pcc::matchClusters: the cluster-matching loop that follows it (:1296-1366) in ONE library call (pcc_cluster_matching).
#pragma once
#include <array>
#include <cstdint>
#include <limits>
#include <vector>
#include "pcc/rift.hpp"
#include "pcc/sift.hpp"

namespace pcc {

struct ClusterDescriptors {
    std::vector<PointCloud<RIFT32>::Ptr> descriptors;  // per cluster
    std::vector<std::vector<int>> point_indices;       // per cluster: the index IN THE CLUSTER of the point every descriptor was
                                                       // computed at (on the SIFT route: the point its keypoint snapped to)
    std::vector<size_t> n_keypoints;                   // per cluster: what processSift found (the reference prints it); 0 on the dense route
    std::vector<PointXYZ> centroids;                   // per cluster: the reference's float sums in index order / float(n); empty: NaN
};

constexpr size_t SIFT_ABOVE = 700;                                        // reference src/comparator.cpp:1228
constexpr size_t SIFT_NEVER = std::numeric_limits<size_t>::max();         // every cluster the dense route (the run without --sift)

// clusters: null or empty ones are empty clusters.  ctx (nullable): any tree whose handle may serve as the call's context; the
// cloud it indexes is not read.
inline ClusterDescriptors clusterDescriptors(const std::vector<PointCloud<PointXYZRGB>::Ptr>& clusters, size_t sift_above = SIFT_ABOVE,
                                             search::KdTree<PointXYZRGB>* ctx = nullptr) {
    const size_t nc = clusters.size();
    ClusterDescriptors out;
    out.descriptors.resize(nc);
    for (PointCloud<RIFT32>::Ptr& d : out.descriptors) d.reset(new PointCloud<RIFT32>);
    out.point_indices.assign(nc, std::vector<int>());
    out.n_keypoints.assign(nc, 0);
    out.centroids.resize(nc);
    if (nc == 0) return out;  // (no library call)
    // the clusters one behind the other: what the segmentation calls leave behind as out_cluster_points / out_offsets
    std::vector<size_t> offsets(nc + 1, 0);
    for (size_t c = 0; c < nc; ++c) offsets[c + 1] = offsets[c] + (clusters[c] ? clusters[c]->size() : 0);
    std::vector<PointXYZRGB> all;
    all.reserve(offsets[nc]);
    for (size_t c = 0; c < nc; ++c)
        if (clusters[c]) all.insert(all.end(), clusters[c]->points.begin(), clusters[c]->points.end());
    const size_t total = all.size();
    std::vector<size_t> out_offsets(nc + 1, 0);
    std::vector<uint32_t> n_kp(nc, 0);
    std::vector<float> centroids(nc * 3, 0.f), hist;
    std::vector<int32_t> index;
    pcc_index* context = detail::batchContext<PointXYZRGB>(ctx ? ctx->handle() : nullptr);
    size_t capacity = total / 4 + 256;
    for (int attempt = 0; attempt < 2; ++attempt) {
        hist.resize(capacity * 32);
        index.resize(capacity);
        const int st = pcc_cluster_descriptors(context, total ? &all[0].x : nullptr, sizeof(PointXYZRGB), total ? &all[0].rgba : nullptr,
                                               sizeof(PointXYZRGB), offsets.data(), nc, PCC_MEM_HOST, sift_above, SIFT_MIN_SCALE, SIFT_NR_OCTAVES,
                                               SIFT_NR_SCALES_PER_OCTAVE, SIFT_MIN_CONTRAST, 0.05, 0.03, 0.03, 0.05, 4, 8, hist.data(), index.data(),
                                               capacity, out_offsets.data(), n_kp.data(), centroids.data());
        if (st == PCC_ERR_OVERFLOW && attempt == 0) { capacity = out_offsets[nc]; continue; }
        check(st);
        break;
    }
    for (size_t c = 0; c < nc; ++c) {
        const size_t m = out_offsets[c + 1] - out_offsets[c];
        PointCloud<RIFT32>& d = *out.descriptors[c];
        d.points.resize(m);
        for (size_t i = 0; i < m; ++i)
            for (int b = 0; b < 32; ++b) d.points[i].histogram[b] = hist[(out_offsets[c] + i) * 32 + b];
        d.width = (std::uint32_t)m;
        d.height = 1;
        d.is_dense = true;
        out.point_indices[c].assign(index.begin() + out_offsets[c], index.begin() + out_offsets[c + 1]);
        out.n_keypoints[c] = n_kp[c];
        out.centroids[c].x = centroids[c * 3];
        out.centroids[c].y = centroids[c * 3 + 1];
        out.centroids[c].z = centroids[c * 3 + 2];
    }
    return out;
}

// ---- the cluster-matching loop (src/comparator.cpp:1296-1366) in one call ------------------------------------------------------
// Per cluster i of scene 1 (pcc_nn.h: pcc_cluster_matching): the three nearest free clusters of scene 2 by centroid (-1: none),
// what became of each (0 no candidate, 1 gated out by the descriptor counts, 2 gated out by size, 3 searched), the length of the
// row matchRIFTFeaturesKnn would return for a searched pair (else 0), and the accepted match (-1: none).
struct ClusterMatches {
    std::vector<std::array<int, 3> > candidates, state;
    std::vector<std::array<uint32_t, 3> > correspondences;
    std::vector<int> matches;
};

// des_s[c]: the descriptors of cluster c of scene s (null: none); centroids_s and points_s: its centroid and its number of
// points.  dims: the bins the search reads (3 = the reference's PCL, 32 = the whole histogram).  ctx (nullable): as above.
inline ClusterMatches matchClusters(const std::vector<PointCloud<RIFT32>::Ptr>& des1, const std::vector<PointCloud<RIFT32>::Ptr>& des2,
                                    const std::vector<std::array<float, 3> >& centroids1, const std::vector<std::array<float, 3> >& centroids2,
                                    const std::vector<size_t>& points1, const std::vector<size_t>& points2, int dims = 3, float threshold = 0.05f,
                                    search::KdTree<PointXYZRGB>* ctx = nullptr) {
    const size_t nc1 = des1.size(), nc2 = des2.size();
    if (centroids1.size() != nc1 || points1.size() != nc1 || centroids2.size() != nc2 || points2.size() != nc2)
        throw Error(PCC_ERR_INVALID, "matchClusters: one centroid and one point count per cluster");
    ClusterMatches out;
    out.candidates.resize(nc1);
    out.state.resize(nc1);
    out.correspondences.resize(nc1);
    out.matches.assign(nc1, -1);
    if (nc1 == 0) return out;  // (no library call)
    std::vector<RIFT32> all[2];
    std::vector<size_t> offsets[2];
    for (int s = 0; s < 2; ++s) {
        const std::vector<PointCloud<RIFT32>::Ptr>& des = s ? des2 : des1;
        offsets[s].assign(des.size() + 1, 0);
        for (size_t c = 0; c < des.size(); ++c) offsets[s][c + 1] = offsets[s][c] + (des[c] ? des[c]->size() : 0);
        all[s].reserve(offsets[s].back());
        for (size_t c = 0; c < des.size(); ++c)
            if (des[c]) all[s].insert(all[s].end(), des[c]->points.begin(), des[c]->points.end());
    }
    std::vector<int32_t> matches(nc1);
    static_assert(sizeof(std::array<int, 3>) == 3 * sizeof(int32_t) && sizeof(std::array<float, 3>) == 3 * sizeof(float), "rows of three");
    check(pcc_cluster_matching(detail::batchContext<PointXYZRGB>(ctx ? ctx->handle() : nullptr), all[0].empty() ? nullptr : all[0].data(),
                               offsets[0].data(), nc1, all[1].empty() ? nullptr : all[1].data(), offsets[1].data(), nc2, sizeof(RIFT32), dims,
                               PCC_MEM_HOST, centroids1[0].data(), nc2 ? centroids2[0].data() : nullptr, points1.data(),
                               nc2 ? points2.data() : nullptr, threshold, out.candidates[0].data(), out.state[0].data(),
                               out.correspondences[0].data(), matches.data()));
    out.matches.assign(matches.begin(), matches.end());
    return out;
}

}  // namespace pcc
