// shot.hpp -- pcc::processSHOT: the deterministic part of the reference's processSHOT (src/comparator.cpp:941-986) re-hosted on
// libpcc_nn.  Same radii (normals 0.05, SHOT 0.04) as the reference; the whole pipeline -- normals, removal of NaN normals, the
// local reference frames and the 352 bins -- is one pcc_shot_descriptors call on a tree over the cloud.  It prints the line the
// reference prints and keeps its fallback (:977-985): an empty result becomes one all-zero descriptor.
// Lines 915-939 of the reference's function -- processSift, the rand() % total draw among the first tenth of the keypoints and
// the snap of every drawn keypoint to the first cloud point within 0.01 -- stay with the caller: pcc::processSift
// (pcc_sift_keypoints) and pcc_first_within cover the two library steps, the draw is the caller's business, and the cloud
// handed over here is the reference's cloud_Color.
#pragma once
#include <iostream>
#include <vector>
#include "pcc/search.hpp"

namespace pcc {

// pcl::SHOT352: the 32 volumes x 11 bins, and the local reference frame (x, y and z axis)
struct SHOT352 {
    float descriptor[352];
    float rf[9];
};

// point_indices (nullable): the index in `cloud` of the point every returned descriptor belongs to (PCL does not say); empty
// when the fallback descriptor is returned
inline PointCloud<SHOT352>::Ptr processSHOT(const PointCloud<PointXYZRGB>::Ptr& cloud, std::vector<int>* point_indices = nullptr,
                                            search::KdTree<PointXYZRGB>* tree = nullptr) {
    PointCloud<SHOT352>::Ptr descriptors(new PointCloud<SHOT352>);
    if (point_indices) point_indices->clear();
    size_t n_out = 0;
    search::KdTree<PointXYZRGB> local;
    if (cloud && !cloud->empty()) {
        if (!tree) { local.setInputCloud(cloud); tree = &local; }
        if (tree->handle()) {  // (no handle: no finite point)
            const size_t n = cloud->size();
            std::vector<float> desc(n * 352), rf(n * 9);
            std::vector<int32_t> index(n);
            check(pcc_shot_descriptors(tree->handle(), PCC_MEM_HOST, 0.05, 0.04, desc.data(), rf.data(), index.data(), &n_out));
            descriptors->points.resize(n_out);
            for (size_t i = 0; i < n_out; ++i) {
                SHOT352& d = descriptors->points[i];
                for (int b = 0; b < 352; ++b) d.descriptor[b] = desc[i * 352 + b];
                for (int k = 0; k < 9; ++k) d.rf[k] = rf[i * 9 + k];
            }
            if (point_indices) point_indices->assign(index.begin(), index.begin() + n_out);
        }
    }
    std::cout << "Point cloud normals size after removing NaNs: " << n_out << std::endl;
    if (descriptors->points.empty()) {  // (:977-985)
        SHOT352 des;
        for (int i = 0; i < 352; ++i) {
            des.descriptor[i] = 0;
            if (i < 9) des.rf[i] = 0;
        }
        descriptors->points.push_back(des);
    }
    descriptors->width = (std::uint32_t)descriptors->points.size();
    descriptors->height = 1;
    descriptors->is_dense = true;
    return descriptors;
}

}  // namespace pcc
