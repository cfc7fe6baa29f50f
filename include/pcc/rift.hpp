// rift.hpp -- pcc::processRIFT: the reference's processRIFT (src/comparator.cpp:590-684) re-hosted on libpcc_nn.
// Same signature, radii (normals 0.03, intensity gradient 0.03, RIFT 0.05) and bins (4 distance x 8 gradient) as the
// reference; the whole pipeline -- intensity, normals, removal of NaN normals, intensity gradient, RIFT, removal of
// non-finite descriptors -- is one pcc_rift_descriptors call on a tree over the cloud.  The reference sends clusters
// above 700 points through SIFT keypoints first (processRIFTwithSIFT, :1228-1231): that route is pcc::processRIFTwithSIFT
// in pcc/sift.hpp, which ends in this function on the snapped keypoint cloud.
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

}  // namespace pcc
