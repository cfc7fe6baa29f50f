// ground.hpp -- the morphological ground filter of the reference's ground_segmentation (src/segmentation.cpp:330-387) with
// PCL's names over libpcc_nn: pcc::applyMorphologicalOperator (pcl::applyMorphologicalOperator), pcc::ProgressiveMorphologicalFilter
// (PCL's setters and extract) and pcc::groundSegmentation, the reference function in one library call.  Header-only; the work is
// pcc_morphological_operator, pcc_progressive_morphological_filter and pcc_ground_segmentation (include/pcc_nn.h).
#pragma once
#include <cstdint>
#include <vector>
#include "pcc/search.hpp"

namespace pcc {

enum MorphologicalOperators { MORPH_OPEN, MORPH_CLOSE, MORPH_DILATE, MORPH_ERODE };  // PCL's names and order

namespace ground_detail {
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
inline int op_of(int morphological_operator) {
    switch (morphological_operator) {
        case MORPH_OPEN: return PCC_MORPH_OPEN;
        case MORPH_CLOSE: return PCC_MORPH_CLOSE;
        case MORPH_DILATE: return PCC_MORPH_DILATE;
        case MORPH_ERODE: return PCC_MORPH_ERODE;
        default: return -1;  // (the library refuses it)
    }
}
}  // namespace ground_detail

// pcl::applyMorphologicalOperator: cloud_out = cloud_in with z replaced by the operator's result over boxes of side `resolution`
template <class PointT>
inline void applyMorphologicalOperator(const typename PointCloud<PointT>::ConstPtr& cloud_in, float resolution, int morphological_operator,
                                       PointCloud<PointT>& cloud_out) {
    if (cloud_in->empty()) { cloud_out = *cloud_in; return; }
    std::vector<float> z(cloud_in->size());
    check(pcc_morphological_operator(ground_detail::context(), cloud_in->points.data(), cloud_in->size(), sizeof(PointT), PCC_MEM_HOST,
                                     resolution, ground_detail::op_of(morphological_operator), z.data()));
    cloud_out = *cloud_in;
    for (size_t i = 0; i < z.size(); ++i) cloud_out.points[i].z = z[i];
}

// pcl::ProgressiveMorphologicalFilter with PCL's defaults
template <class PointT>
class ProgressiveMorphologicalFilter {
public:
    void setInputCloud(const typename PointCloud<PointT>::ConstPtr& cloud) { input_ = cloud; }
    void setMaxWindowSize(int v) { max_window_size_ = v; }
    void setSlope(float v) { slope_ = v; }
    void setMaxDistance(float v) { max_distance_ = v; }
    void setInitialDistance(float v) { initial_distance_ = v; }
    void setCellSize(float v) { cell_size_ = v; }
    void setBase(float v) { base_ = v; }
    void setExponential(bool v) { exponential_ = v; }
    int getMaxWindowSize() const { return max_window_size_; }
    float getSlope() const { return slope_; }
    float getMaxDistance() const { return max_distance_; }
    float getInitialDistance() const { return initial_distance_; }
    float getCellSize() const { return cell_size_; }
    float getBase() const { return base_; }
    bool getExponential() const { return exponential_; }
    // the survivors after each window of the last extract
    const std::vector<size_t>& getPassSizes() const { return pass_sizes_; }

    void extract(std::vector<int>& ground) {
        ground.clear();
        pass_sizes_.clear();
        if (!input_ || input_->empty()) return;
        std::vector<int32_t> idx(input_->size());
        size_t ng = 0;
        pass_sizes_.assign(PCC_PMF_MAX_WINDOWS, 0);
        check(pcc_progressive_morphological_filter(ground_detail::context(), input_->points.data(), input_->size(), sizeof(PointT),
                                                   PCC_MEM_HOST, max_window_size_, slope_, initial_distance_, max_distance_, cell_size_,
                                                   base_, exponential_ ? 1 : 0, idx.data(), &ng, pass_sizes_.data(), pass_sizes_.size()));
        float w[PCC_PMF_MAX_WINDOWS], h[PCC_PMF_MAX_WINDOWS];
        size_t nw = 0;
        check(pcc_pmf_windows(max_window_size_, slope_, initial_distance_, max_distance_, cell_size_, base_, exponential_ ? 1 : 0,
                              PCC_PMF_MAX_WINDOWS, w, h, &nw));
        pass_sizes_.resize(nw);
        ground.assign(idx.begin(), idx.begin() + (std::ptrdiff_t)ng);
    }

private:
    typename PointCloud<PointT>::ConstPtr input_;
    int max_window_size_ = 33;
    float slope_ = 0.7f, max_distance_ = 10.0f, initial_distance_ = 0.15f, cell_size_ = 1.0f, base_ = 2.0f;
    bool exponential_ = true;
    std::vector<size_t> pass_sizes_;
};

// ground_segmentation (src/segmentation.cpp:330-387) in one library call: VoxelGrid leaf -> ProgressiveMorphologicalFilter ->
// ExtractIndices, positive (*ground) and negative (*object); the defaults are the reference's.  *filtered (may be null)
// receives the filtered cloud, *ground_index (may be null) the ground's indices into it.
template <class PointT>
inline void groundSegmentation(const typename PointCloud<PointT>::ConstPtr& cloud, PointCloud<PointT>& ground, PointCloud<PointT>& object,
                               float leaf = 0.01f, int max_window_size = 20, float slope = 1.0f, float initial_distance = 0.5f,
                               float max_distance = 3.0f, float cell_size = 1.0f, float base = 2.0f, bool exponential = true,
                               PointCloud<PointT>* filtered = nullptr, std::vector<int>* ground_index = nullptr) {
    ground = PointCloud<PointT>();
    object = PointCloud<PointT>();
    if (filtered) *filtered = PointCloud<PointT>();
    if (ground_index) ground_index->clear();
    if (!cloud || cloud->empty()) return;
    const size_t n = cloud->size();
    std::vector<PointT> f(n), g(n), o(n);
    std::vector<int32_t> idx(n);
    size_t nv = 0, ng = 0;
    if (n >= (1ull << 31)) throw Error(PCC_ERR_UNSUPPORTED, "groundSegmentation: more than 2^31 points");
    const int st = pcc_ground_segmentation(ground_detail::context(), cloud->points.data(), n, sizeof(PointT), PCC_MEM_HOST, leaf,
                                           max_window_size, slope, initial_distance, max_distance, cell_size, base, exponential ? 1 : 0,
                                           f.data(), sizeof(PointT), &nv, idx.data(), &ng, g.data(), o.data());
    if (st == PCC_ERR_UNSUPPORTED) {
        // the leaf is too small for the cloud's extent (the reference's 0.01 over an airborne tile).  PCL's VoxelGrid warns and
        // hands its input on: the filter runs over the cloud as it is
        f = cloud->points;
        nv = n;
        check(pcc_progressive_morphological_filter(ground_detail::context(), f.data(), n, sizeof(PointT), PCC_MEM_HOST, max_window_size, slope,
                                                   initial_distance, max_distance, cell_size, base, exponential ? 1 : 0, idx.data(), &ng,
                                                   nullptr, 0));
        size_t next = 0, no = 0;
        for (size_t i = 0; i < n; ++i) {
            if (next < ng && (size_t)idx[next] == i) g[next++] = f[i];
            else o[no++] = f[i];
        }
    } else {
        check(st);
    }
    auto fill = [](PointCloud<PointT>& c, std::vector<PointT>& pts, size_t count) {
        pts.resize(count);
        c.points.swap(pts);
        c.width = (std::uint32_t)count;
        c.height = 1;
        c.is_dense = true;
    };
    fill(ground, g, ng);
    fill(object, o, nv - ng);
    if (filtered) fill(*filtered, f, nv);
    if (ground_index) ground_index->assign(idx.begin(), idx.begin() + (std::ptrdiff_t)ng);
}

}  // namespace pcc
