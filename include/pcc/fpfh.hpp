// fpfh.hpp -- pcc::processFPFH: the reference's processFPFH (src/comparator.cpp:824-875) re-hosted on libpcc_nn.
// Same signature, radii (normals 0.03, FPFH 0.05) and bins (11 + 11 + 11) as the reference; the whole pipeline -- normals,
// removal of NaN normals, the SPFH signatures and their weighted sums -- is one pcc_fpfh_descriptors call on a tree over the
// cloud.  It prints the two lines the reference prints.  (The reference's matchFPFH, a 33-dimensional search, has no
// counterpart yet.)
#pragma once
#include <iostream>
#include <vector>
#include "pcc/search.hpp"

namespace pcc {

// pcl::FPFHSignature33: the eleven bins of f1, of f2 and of f3
struct FPFHSignature33 {
    float histogram[33];
};

// point_indices (nullable): the index in `cloud` of the point every returned descriptor belongs to (PCL does not say)
inline PointCloud<FPFHSignature33>::Ptr processFPFH(const PointCloud<PointXYZRGB>::Ptr& cloud, std::vector<int>* point_indices = nullptr,
                                                    search::KdTree<PointXYZRGB>* tree = nullptr) {
    PointCloud<FPFHSignature33>::Ptr descriptors(new PointCloud<FPFHSignature33>);
    if (point_indices) point_indices->clear();
    size_t n_out = 0;
    search::KdTree<PointXYZRGB> local;
    if (cloud && !cloud->empty()) {
        if (!tree) { local.setInputCloud(cloud); tree = &local; }
        if (tree->handle()) {  // (no handle: no finite point)
            const size_t n = cloud->size();
            descriptors->points.resize(n);
            std::vector<int32_t> index(n);
            check(pcc_fpfh_descriptors(tree->handle(), PCC_MEM_HOST, 0.03, 0.05, 11, 11, 11, descriptors->points[0].histogram, index.data(), &n_out));
            if (point_indices) point_indices->assign(index.begin(), index.begin() + n_out);
        }
    }
    descriptors->points.resize(n_out);
    descriptors->width = (std::uint32_t)n_out;
    descriptors->height = 1;
    descriptors->is_dense = true;
    std::cout << "Point cloud normals size after removing NaNs: " << n_out << std::endl;
    std::cout << "Computed " << descriptors->points.size() << " FPFH descriptors" << std::endl;
    return descriptors;
}

}  // namespace pcc
