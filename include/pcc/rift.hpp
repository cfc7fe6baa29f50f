// rift.hpp -- pcc::processRIFT: the reference's processRIFT (src/comparator.cpp:590-684) re-hosted on libpcc_nn.
// Same signature, radii (normals 0.03, intensity gradient 0.03, RIFT 0.05) and bins (4 distance x 8 gradient) as the
// reference; the whole pipeline -- intensity, normals, removal of NaN normals, intensity gradient, RIFT, removal of
// non-finite descriptors -- is one pcc_rift_descriptors call on a tree over the cloud.  The reference sends clusters
// above 700 points through SIFT keypoints first (processRIFTwithSIFT, :1228-1231): that route is pcc::processRIFTwithSIFT
// in pcc/sift.hpp, which ends in this function on the snapped keypoint cloud.
// pcc::processRIFTBatch is the same for every cluster of a comparison at once (the reference's per-cluster loop,
// src/comparator.cpp:1224-1272): one pcc_rift_descriptors_batch call.
#pragma once
#include <vector>
#include "pcc/search.hpp"

namespace pcc {

typedef Histogram<32> RIFT32;  // reference src/comparator.cpp:9

// point_indices (nullable): the index in `cloud` of the point every returned descriptor belongs to (PCL does not say)
inline PointCloud<RIFT32>::Ptr processRIFT(const PointCloud<PointXYZRGB>::Ptr& cloud, std::vector<int>* point_indices = nullptr,
                                           search::KdTree<PointXYZRGB>* tree = nullptr) {
    PointCloud<RIFT32>::Ptr descriptors(new PointCloud<RIFT32>);
    if (point_indices) point_indices->clear();
    if (!cloud || cloud->empty()) return descriptors;
    search::KdTree<PointXYZRGB> local;
    if (!tree) { local.setInputCloud(cloud); tree = &local; }
    if (!tree->handle()) return descriptors;  // no finite point
    const size_t n = cloud->size();
    descriptors->points.resize(n);
    std::vector<int32_t> index(n);
    size_t n_out = 0;
    check(pcc_rift_descriptors(tree->handle(), &cloud->points[0].rgba, sizeof(PointXYZRGB), PCC_MEM_HOST, 0.03, 0.03, 0.05, 4, 8,
                               descriptors->points[0].histogram, index.data(), &n_out));
    descriptors->points.resize(n_out);
    descriptors->width = (std::uint32_t)n_out;
    descriptors->height = 1;
    descriptors->is_dense = true;
    if (point_indices) point_indices->assign(index.begin(), index.begin() + n_out);
    return descriptors;
}

// processRIFT for every cloud of `clouds` in ONE library call: element c of the result is what processRIFT(clouds[c])
// returns, bit for bit (a null or empty cloud, or one without a finite point, gives empty descriptors).
// point_indices (nullable): per cloud, the index in that cloud of the point every returned descriptor belongs to.
// ctx (nullable): any tree whose handle may serve as the call's context; the cloud it indexes is not read.
inline std::vector<PointCloud<RIFT32>::Ptr> processRIFTBatch(const std::vector<PointCloud<PointXYZRGB>::Ptr>& clouds,
                                                             std::vector<std::vector<int>>* point_indices = nullptr,
                                                             search::KdTree<PointXYZRGB>* ctx = nullptr) {
    std::vector<PointCloud<RIFT32>::Ptr> result(clouds.size());
    for (PointCloud<RIFT32>::Ptr& d : result) d.reset(new PointCloud<RIFT32>);
    if (point_indices) point_indices->assign(clouds.size(), std::vector<int>());
    const detail::BatchClouds b(clouds);
    const size_t total = b.total();
    if (total == 0) return result;  // (no library call)
    std::vector<size_t> offsets(clouds.size() + 1, 0);
    std::vector<float> hist(total * 32);
    std::vector<int32_t> index(total);
    check(pcc_rift_descriptors_batch(detail::batchContext<PointXYZRGB>(ctx ? ctx->handle() : nullptr), clouds.size(), b.pts.data(), b.n.data(),
                                     sizeof(PointXYZRGB), b.rgb.data(), sizeof(PointXYZRGB), PCC_MEM_HOST, 0.03, 0.03, 0.05, 4, 8, hist.data(),
                                     index.data(), offsets.data()));
    for (size_t c = 0; c < clouds.size(); ++c) {
        const size_t m = offsets[c + 1] - offsets[c];
        PointCloud<RIFT32>& d = *result[c];
        d.points.resize(m);
        for (size_t i = 0; i < m; ++i)
            for (int b = 0; b < 32; ++b) d.points[i].histogram[b] = hist[(offsets[c] + i) * 32 + b];
        d.width = (std::uint32_t)m;
        d.height = 1;
        d.is_dense = true;
        if (point_indices) (*point_indices)[c].assign(index.begin() + offsets[c], index.begin() + offsets[c + 1]);
    }
    return result;
}

}  // namespace pcc
