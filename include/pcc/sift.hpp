// sift.hpp -- pcc::processSift and pcc::processRIFTwithSIFT: the reference's processSift (src/comparator.cpp:435-469) and
// processRIFTwithSIFT (:686-822) re-hosted on libpcc_nn.  The reference sends every cluster above 700 points through the
// second (:1228-1231, :1264-1265): SIFT keypoints of the cluster, each snapped to the first cluster point within 0.05
// (:696-713), then the RIFT pipeline over the snapped cloud -- a few dozen descriptors at keypoints instead of thousands of
// dense ones.
//   processSift          pcl::SIFTKeypoint<PointXYZRGB, PointWithScale>, setScales(0.005f, 5, 5), setMinimumContrast(0.001f):
//                        one pcc_sift_keypoints call
//   processRIFTwithSIFT  processSift -> snapKeypointsToCloud (pcc_first_within; keypoints without a point within 0.05 are
//                        skipped, duplicates are kept) -> a tree over the snapped cloud -> processRIFT on it
//   siftSnappedCloud     the part of processRIFTwithSIFT in front of processRIFT: the snapped keypoint cloud, for callers
//                        that hand it to pcc::processRIFTBatch with other clouds
#pragma once
#include <vector>
#include "pcc/comparator_nn.hpp"
#include "pcc/rift.hpp"

namespace pcc {

constexpr float SIFT_MIN_SCALE = 0.005f;      // reference src/comparator.cpp:435-469
constexpr int SIFT_NR_OCTAVES = 5;
constexpr int SIFT_NR_SCALES_PER_OCTAVE = 5;
constexpr float SIFT_MIN_CONTRAST = 0.001f;

// tree (nullable): any tree whose handle may serve as the call's context; the cloud it indexes is not read
inline PointCloud<PointWithScale>::Ptr processSift(const PointCloud<PointXYZRGB>::Ptr& cloud, search::KdTree<PointXYZRGB>* tree = nullptr) {
    PointCloud<PointWithScale>::Ptr keypoints(new PointCloud<PointWithScale>);
    if (!cloud || cloud->empty()) return keypoints;
    search::KdTree<PointXYZRGB> local;
    if (!tree || !tree->handle()) { local.setInputCloud(cloud); tree = &local; }
    if (!tree->handle()) return keypoints;  // no finite point
    const size_t n = cloud->size();
    std::vector<float> out;
    size_t capacity = 256, found = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        out.resize(capacity * 4);
        const int st = pcc_sift_keypoints(tree->handle(), &cloud->points[0].x, n, sizeof(PointXYZRGB), &cloud->points[0].rgba, sizeof(PointXYZRGB),
                                          PCC_MEM_HOST, SIFT_MIN_SCALE, SIFT_NR_OCTAVES, SIFT_NR_SCALES_PER_OCTAVE, SIFT_MIN_CONTRAST, out.data(),
                                          capacity, &found);
        if (st == PCC_ERR_OVERFLOW && attempt == 0) { capacity = found; continue; }
        check(st);
        break;
    }
    keypoints->points.resize(found);
    for (size_t i = 0; i < found; ++i) {
        PointWithScale& k = keypoints->points[i];
        k.x = out[i * 4]; k.y = out[i * 4 + 1]; k.z = out[i * 4 + 2]; k.scale = out[i * 4 + 3];
    }
    keypoints->width = (std::uint32_t)found;
    keypoints->height = 1;
    return keypoints;
}

// the front of processRIFTwithSIFT: processSift, then every keypoint snapped to the first point of `cloud` within 0.05 (:696-713).
// The snapped cloud is what the RIFT pipeline runs over (processRIFT, or one entry of processRIFTBatch).
// n_keypoints (nullable): what processSift found (the reference prints it)
inline PointCloud<PointXYZRGB>::Ptr siftSnappedCloud(const PointCloud<PointXYZRGB>::Ptr& cloud, size_t* n_keypoints = nullptr) {
    if (n_keypoints) *n_keypoints = 0;
    if (!cloud || cloud->empty()) return PointCloud<PointXYZRGB>::Ptr(new PointCloud<PointXYZRGB>);
    search::KdTree<PointXYZRGB> tree;
    tree.setInputCloud(cloud);
    const PointCloud<PointWithScale>::Ptr keypoints = processSift(cloud, &tree);
    if (n_keypoints) *n_keypoints = keypoints->size();
    return snapKeypointsToCloud(cloud, *keypoints, 0.05, &tree);
}

// point_indices (nullable): the index in the SNAPPED cloud of the point every returned descriptor belongs to;
// n_keypoints (nullable): what processSift found (the reference prints it)
inline PointCloud<RIFT32>::Ptr processRIFTwithSIFT(const PointCloud<PointXYZRGB>::Ptr& cloud, std::vector<int>* point_indices = nullptr,
                                                   size_t* n_keypoints = nullptr) {
    if (point_indices) point_indices->clear();
    if (n_keypoints) *n_keypoints = 0;
    if (!cloud || cloud->empty()) return PointCloud<RIFT32>::Ptr(new PointCloud<RIFT32>);
    return processRIFT(siftSnappedCloud(cloud, n_keypoints), point_indices);
}

}  // namespace pcc
