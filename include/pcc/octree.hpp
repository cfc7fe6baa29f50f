// octree.hpp -- pcl::octree::OctreePointCloudChangeDetector with PCL's names over libpcc_nn, as the reference's
// spatial_change_detection uses it (src/comparator.cpp:54-110, called from both verdict branches of main, :1687-1698), and
// pcc::spatialChangeDetection, that function's work in one library call.  Header-only; the work is pcc_change_detection
// (include/pcc_nn.h), whose comment holds the contract: the voxel lattice the first finite point of the first cloud fixes, the
// points of the second cloud in voxels the first leaves empty, indices ASCENDING (PCL: octree traversal order).
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>
#include "pcc/search.hpp"

namespace pcc {

namespace octree_detail {
// any index handle supplies device, stream and scratch; a one-point index is the cheapest.  One per thread, kept.
inline pcc_index* context() {
    struct Context {
        pcc_index* h = nullptr;
        ~Context() { if (h) pcc_index_destroy(h); }
    };
    static thread_local Context context;
    if (!context.h) {
        const float one[3] = {0.f, 0.f, 0.f};
        check(pcc_index_create(one, 1, 12, 3, PCC_MEM_HOST, 0, PCC_ENGINE_BRUTE, &context.h));
    }
    return context.h;
}

// the points of b in voxels a leaves empty: their indices and, with `records`, the points themselves.  No buffer behind b
// (nothing was added before switchBuffers): PCL finds every voxel new -- a single non-finite point stands in for the empty cloud
template <class PointT>
inline void detect(const PointCloud<PointT>* a, const PointCloud<PointT>& b, double resolution, int min_points_per_leaf,
                   std::vector<int>& indices, std::vector<PointT>* records) {
    indices.clear();
    if (records) records->clear();
    if (b.empty()) return;
    PointT none;
    float* c = reinterpret_cast<float*>(&none);
    c[0] = c[1] = c[2] = std::numeric_limits<float>::quiet_NaN();
    const bool have_a = a && !a->empty();
    std::vector<int32_t> idx(b.size());
    if (records) records->resize(b.size());
    size_t n = 0;
    check(pcc_change_detection(context(), have_a ? a->points.data() : &none, have_a ? a->size() : 1, sizeof(PointT), b.points.data(),
                               b.size(), sizeof(PointT), PCC_MEM_HOST, resolution, min_points_per_leaf, idx.data(),
                               records ? records->data() : nullptr, &n));
    indices.assign(idx.begin(), idx.begin() + (std::ptrdiff_t)n);
    if (records) records->resize(n);
}
}  // namespace octree_detail

namespace octree {

// The reference's sequence: setInputCloud(A); addPointsFromInputCloud(); switchBuffers(); setInputCloud(B);
// addPointsFromInputCloud(); getPointIndicesFromNewVoxels(v).  The object records the two clouds -- the one added before the last
// switchBuffers and the one added since -- and issues the one library call at getPointIndicesFromNewVoxels.
template <class PointT>
class OctreePointCloudChangeDetector {
public:
    typedef typename PointCloud<PointT>::ConstPtr PointCloudConstPtr;
    explicit OctreePointCloudChangeDetector(double resolution) : resolution_(resolution) {}
    void setInputCloud(const PointCloudConstPtr& cloud) { input_ = cloud; }
    void addPointsFromInputCloud() { current_ = input_; }
    void switchBuffers() { previous_ = current_; current_.reset(); }
    double getResolution() const { return resolution_; }
    void setResolution(double resolution) { resolution_ = resolution; }
    // the indices (into the cloud added since switchBuffers) of the points in voxels the previous buffer did not have and that
    // hold at least min_points_per_leaf points, ascending; returns their number
    std::size_t getPointIndicesFromNewVoxels(std::vector<int>& indices, int min_points_per_leaf = 0) {
        indices.clear();
        if (!current_) return 0;
        octree_detail::detect<PointT>(previous_.get(), *current_, resolution_, min_points_per_leaf, indices, nullptr);
        return indices.size();
    }

private:
    double resolution_;
    PointCloudConstPtr input_, current_, previous_;
};

}  // namespace octree

// spatial_change_detection (src/comparator.cpp:54-110) behind its file reading and before its viewer: the cloud of the points of
// cloudB that lie in voxels of side `resolution` (the reference: 32) holding no point of cloudA, whole records (the colour
// with them), in cloudB's order.  *indices (may be null) receives their indices into cloudB.
template <class PointT>
inline typename PointCloud<PointT>::Ptr spatialChangeDetection(const typename PointCloud<PointT>::ConstPtr& cloudA,
                                                               const typename PointCloud<PointT>::ConstPtr& cloudB, double resolution = 32.0,
                                                               std::vector<int>* indices = nullptr, int min_points_per_leaf = 0) {
    typename PointCloud<PointT>::Ptr diff(new PointCloud<PointT>);
    std::vector<int> idx;
    if (cloudB) octree_detail::detect<PointT>(cloudA.get(), *cloudB, resolution, min_points_per_leaf, idx, &diff->points);
    diff->width = (std::uint32_t)diff->points.size();
    diff->height = 1;
    diff->is_dense = true;
    if (indices) indices->swap(idx);
    return diff;
}

}  // namespace pcc
