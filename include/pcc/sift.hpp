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
//   processSiftBatch / siftSnappedCloudBatch   processSift / siftSnappedCloud for every cluster of a comparison in ONE
//                        library call (pcc_sift_keypoints_batch): the reference's loop over the clusters above 700 points
//                        (:1228-1231, :1264-1265), no turn of which depends on an earlier one
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

namespace detail {
// one pcc_sift_keypoints_batch call over `clouds` (null or empty ones are empty clouds of the batch); snap (nullable): the snapped
// index of every keypoint at radius 0.05.  ctx (nullable): any tree whose handle may serve as the call's context
inline void siftBatchCall(const std::vector<PointCloud<PointXYZRGB>::Ptr>& clouds, std::vector<float>& keypoints, std::vector<int32_t>* snap,
                          std::vector<size_t>& offsets, search::KdTree<PointXYZRGB>* ctx) {
    const size_t nc = clouds.size();
    offsets.assign(nc + 1, 0);
    keypoints.clear();
    if (snap) snap->clear();
    const BatchClouds b(clouds);
    if (b.total() == 0) return;  // (no library call)
    pcc_index* context = batchContext<PointXYZRGB>(ctx ? ctx->handle() : nullptr);
    size_t capacity = b.total() / 8 + 256;
    for (int attempt = 0; attempt < 2; ++attempt) {
        keypoints.resize(capacity * 4);
        if (snap) snap->resize(capacity);
        const int st = pcc_sift_keypoints_batch(context, nc, b.pts.data(), b.n.data(), sizeof(PointXYZRGB), b.rgb.data(), sizeof(PointXYZRGB),
                                                PCC_MEM_HOST, SIFT_MIN_SCALE, SIFT_NR_OCTAVES, SIFT_NR_SCALES_PER_OCTAVE, SIFT_MIN_CONTRAST, 0.05,
                                                keypoints.data(), snap ? snap->data() : nullptr, capacity, offsets.data());
        if (st == PCC_ERR_OVERFLOW && attempt == 0) { capacity = offsets[nc]; continue; }
        check(st);
        break;
    }
    keypoints.resize(offsets[nc] * 4);
    if (snap) snap->resize(offsets[nc]);
}
}  // namespace detail

// processSift for every cloud of `clouds` in ONE library call: element c of the result is what processSift(clouds[c]) returns, bit
// for bit (a null or empty cloud, or one without a finite point, gives no keypoints).
inline std::vector<PointCloud<PointWithScale>::Ptr> processSiftBatch(const std::vector<PointCloud<PointXYZRGB>::Ptr>& clouds,
                                                                     search::KdTree<PointXYZRGB>* ctx = nullptr) {
    std::vector<PointCloud<PointWithScale>::Ptr> result(clouds.size());
    std::vector<float> kp;
    std::vector<size_t> offsets;
    detail::siftBatchCall(clouds, kp, nullptr, offsets, ctx);
    for (size_t c = 0; c < clouds.size(); ++c) {
        result[c].reset(new PointCloud<PointWithScale>);
        const size_t m = offsets[c + 1] - offsets[c];
        result[c]->points.resize(m);
        for (size_t i = 0; i < m; ++i) {
            PointWithScale& k = result[c]->points[i];
            const float* v = &kp[(offsets[c] + i) * 4];
            k.x = v[0]; k.y = v[1]; k.z = v[2]; k.scale = v[3];
        }
        result[c]->width = (std::uint32_t)m;
        result[c]->height = 1;
    }
    return result;
}

// siftSnappedCloud for every cloud of `clouds` in ONE library call: element c is the snapped keypoint cloud of clouds[c] (keypoints
// without a point within 0.05 are skipped, duplicates are kept, as in snapKeypointsToCloud).
// n_keypoints (nullable): per cloud, what processSift found (the reference prints it)
inline std::vector<PointCloud<PointXYZRGB>::Ptr> siftSnappedCloudBatch(const std::vector<PointCloud<PointXYZRGB>::Ptr>& clouds,
                                                                       std::vector<size_t>* n_keypoints = nullptr,
                                                                       search::KdTree<PointXYZRGB>* ctx = nullptr) {
    std::vector<PointCloud<PointXYZRGB>::Ptr> result(clouds.size());
    std::vector<float> kp;
    std::vector<int32_t> snap;
    std::vector<size_t> offsets;
    detail::siftBatchCall(clouds, kp, &snap, offsets, ctx);
    if (n_keypoints) n_keypoints->assign(clouds.size(), 0);
    for (size_t c = 0; c < clouds.size(); ++c) {
        result[c].reset(new PointCloud<PointXYZRGB>);
        if (n_keypoints) (*n_keypoints)[c] = offsets[c + 1] - offsets[c];
        for (size_t i = offsets[c]; i < offsets[c + 1]; ++i)
            if (snap[i] >= 0) result[c]->push_back(clouds[c]->points[snap[i]]);
    }
    return result;
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
