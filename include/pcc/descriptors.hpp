// descriptors.hpp -- pcc::clusterDescriptors: the reference's per-cluster descriptor loop (src/comparator.cpp:1224-1290) in ONE
// library call (pcc_cluster_descriptors).  A cluster above `sift_above` points (700 in the reference, :1228-1231, :1264-1265)
// gets what pcc::processRIFTwithSIFT returns for it, the others what pcc::processRIFT returns; every cluster's centroid
// (:1235-1247) comes with them.  Neither keypoints nor snapped clouds visit the host in between.
#pragma once
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

}  // namespace pcc
