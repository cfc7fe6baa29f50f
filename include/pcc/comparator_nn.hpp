// comparator_nn.hpp -- host-side mirror of the reference's functions and PCL algorithm objects
// that sit on the nearest-neighbour path, re-hosted on libpcc_nn (same names, argument meaning,
// printed lines and error behaviour):
//   matchRIFTFeaturesKnn            reference src/comparator.cpp:560-588
//   performICP                      reference src/comparator.cpp:1089-1110
//   IterativeClosestPoint           the PCL object performICP drives (:1091-1099)
//   StatisticalOutlierRemoval       the -n noise pass (:1520-1549)
//   EuclideanClusterExtraction      the -e path (src/segmentation.cpp:119-131)
//   removePlanes                    the plane-removal loop in front of it (src/segmentation.cpp:79-117) as one call
//   regionGrowingSegmentation       the default path (src/segmentation.cpp:218-327) as one call
//   euclideanClusterSegmentation    the -e path (src/segmentation.cpp:64-156) as one call
// Everything numerical happens behind the C-ABI; this header is plumbing a maintainer of the
// reference can include instead of the PCL headers for these five call sites.
#pragma once
#include <algorithm>
#include <array>
#include <cfloat>
#include <iostream>
#include "pcc/search.hpp"

namespace pcc {

typedef Histogram<32> RIFT32;  // reference src/comparator.cpp:9

// ---- matchRIFTFeaturesKnn (src/comparator.cpp:560-588) --------------------------------------
// Tree on descriptors1, one k=1 query per element of descriptors2, match kept when
// neighborCount == 1 && d2 < 0.05f.  The returned vector STARTS WITH ONE DUMMY 0 (:568), so
// size() == matches + 1 -- callers divide size() by descriptor counts (:1336-1338).
// dims: the bins of a descriptor the search reads, 1 ... 32.  3 is what the reference's PCL does (pcl::Histogram<32> has no
// point representation of its own; recalled); any other value runs matchRIFTFeaturesKnnBatch on this one pair.
inline std::vector<std::vector<int> > matchRIFTFeaturesKnnBatch(
    const std::vector<std::pair<PointCloud<RIFT32>::Ptr, PointCloud<RIFT32>::Ptr> >& pairs, int dims);
inline std::vector<int> matchRIFTFeaturesKnn(const PointCloud<RIFT32>::Ptr& descriptors1,
                                             const PointCloud<RIFT32>::Ptr& descriptors2, int dims = 3) {
    if (dims != 3)
        return matchRIFTFeaturesKnnBatch(std::vector<std::pair<PointCloud<RIFT32>::Ptr, PointCloud<RIFT32>::Ptr> >(
                                             1, std::make_pair(descriptors1, descriptors2)), dims)[0];
    std::vector<int> correspondence(1);
    // `= new KdTreeFLANN<RIFT32>(false)` in the reference: sorted == true, and one (leaked) tree per
    // call.  Here one tree per thread is re-pointed at each descriptor cloud: the reference calls this
    // up to three times per cluster (:1322) and a fresh device handle per call would cost ~1 ms of
    // allocations for microseconds of work.
    static thread_local KdTreeFLANN<RIFT32> matching;
    // the matched indices go back to the caller (:580): among descriptors at exactly the same distance name the one
    // PCL's FLANN tree would (descriptor clouds are full of duplicates in their first three bins)
    matching.setTieOrder(PCC_TIES_FLANN);
    matching.setInputCloud(descriptors1);
    if (!matching.handle() || !descriptors2 || descriptors2->empty()) return correspondence;
    std::vector<int> out(descriptors2->size() + 1);
    int32_t n = 0;
    check(pcc_match_knn(matching.handle(), descriptors2->points.data(), descriptors2->size(), sizeof(RIFT32),
                        PCC_MEM_HOST, 0.05f, out.data(), &n));
    out.resize(n);
    return out;
}

// ---- every matchRIFTFeaturesKnn call of the cluster-matching loop at once (src/comparator.cpp:1296-1365, call at :1322) ----
// pairs[p] = (descriptors1, descriptors2) of one call; element p of the result is what matchRIFTFeaturesKnn(pairs[p]) returns
// (PCC_TIES_FLANN as there; a null or empty cloud on either side gives the dummy alone).  One pcc_match_knn_batch: one
// upload, one search launch and one wait for all pairs.  No pair at all makes no library call.
// dims: the bins the search reads (pcc_match_knn_batch_dims when not 3: on the whole histogram with 32; exact ties then go to
// the lowest index).
inline std::vector<std::vector<int> > matchRIFTFeaturesKnnBatch(
    const std::vector<std::pair<PointCloud<RIFT32>::Ptr, PointCloud<RIFT32>::Ptr> >& pairs, int dims = 3) {
    std::vector<std::vector<int> > result(pairs.size(), std::vector<int>(1));
    if (pairs.empty()) return result;
    static thread_local KdTreeFLANN<RIFT32> context;  // lends device, stream and scratch; the cloud it indexes is never asked
    if (!context.handle()) {
        PointCloud<RIFT32>::Ptr one(new PointCloud<RIFT32>);
        one->push_back(RIFT32());
        for (float& v : one->points[0].histogram) v = 0.f;
        context.setInputCloud(one);
    }
    context.setTieOrder(PCC_TIES_FLANN);
    std::vector<const void*> d1(pairs.size(), nullptr), d2(pairs.size(), nullptr);
    std::vector<size_t> n1(pairs.size(), 0), n2(pairs.size(), 0), offsets(pairs.size() + 1);
    size_t total = pairs.size();
    for (size_t p = 0; p < pairs.size(); ++p) {
        if (!pairs[p].first || !pairs[p].second || pairs[p].first->empty() || pairs[p].second->empty()) continue;
        d1[p] = pairs[p].first->points.data();
        n1[p] = pairs[p].first->size();
        d2[p] = pairs[p].second->points.data();
        n2[p] = pairs[p].second->size();
        total += n2[p];
    }
    std::vector<int32_t> out(total);
    if (dims == 3)
        check(pcc_match_knn_batch(context.handle(), pairs.size(), d1.data(), n1.data(), d2.data(), n2.data(), sizeof(RIFT32), PCC_MEM_HOST,
                                  0.05f, out.data(), offsets.data()));
    else
        check(pcc_match_knn_batch_dims(context.handle(), pairs.size(), d1.data(), n1.data(), d2.data(), n2.data(), sizeof(RIFT32), dims,
                                       PCC_MEM_HOST, 0.05f, out.data(), nullptr, offsets.data()));
    for (size_t p = 0; p < pairs.size(); ++p) result[p].assign(out.begin() + offsets[p], out.begin() + offsets[p + 1]);
    return result;
}

// ---- pcl::VoxelGrid (src/segmentation.cpp:69-74, 224-229) -------------------------------------------
template <class PointT>
class VoxelGrid {
public:
    void setInputCloud(const typename PointCloud<PointT>::ConstPtr& c) { input_ = c; }
    void setLeafSize(float lx, float ly, float lz) {
        if (lx != ly || ly != lz) throw Error(PCC_ERR_UNSUPPORTED, "anisotropic leaf sizes are not supported");
        leaf_ = lx;
    }
    void filter(PointCloud<PointT>& output) {
        PointCloud<PointT> result;
        if (input_ && !input_->empty()) {
            search::KdTree<PointT> ctx;  // supplies device, stream and scratch
            ctx.setInputCloud(input_);
            if (ctx.handle()) {
                result.points.resize(input_->size());
                size_t nv = 0;
                const int has_rgb = sizeof(PointT) >= 20 ? 1 : 0;
                int st = pcc_voxel_grid(ctx.handle(), input_->points.data(), input_->size(), sizeof(PointT), PCC_MEM_HOST,
                                        leaf_, has_rgb, result.points.data(), sizeof(PointT), &nv);
                if (st == PCC_ERR_UNSUPPORTED) { result = *input_; nv = result.size(); }  // PCL: "leaf size is too small", output = input
                else check(st);
                result.points.resize(nv);
            }
        }
        result.width = (std::uint32_t)result.points.size();
        result.height = 1;
        result.is_dense = true;
        output = result;
    }

private:
    typename PointCloud<PointT>::ConstPtr input_;
    float leaf_ = 0.f;
};

// ---- keypoint snap (src/comparator.cpp:696-713, inside processRIFTwithSIFT) -----------------------
// For every keypoint the FIRST cloud point within `radius` (0.05 in the reference; float differences,
// double-precision distance) is appended to the result, keypoints without one are skipped.
template <class KeyPointT>
inline PointCloud<PointXYZRGB>::Ptr snapKeypointsToCloud(const PointCloud<PointXYZRGB>::Ptr& cloud,
                                                         const PointCloud<KeyPointT>& keypoints, double radius = 0.05,
                                                         search::KdTree<PointXYZRGB>* tree = nullptr) {
    PointCloud<PointXYZRGB>::Ptr out(new PointCloud<PointXYZRGB>);
    if (!cloud || cloud->empty() || keypoints.empty()) return out;
    search::KdTree<PointXYZRGB> local;
    if (!tree) { local.setInputCloud(cloud); tree = &local; }
    if (!tree->handle()) return out;
    std::vector<int32_t> idx(keypoints.size());
    check(pcc_first_within(tree->handle(), keypoints.points.data(), keypoints.size(), sizeof(KeyPointT), PCC_MEM_HOST,
                           radius, idx.data()));
    for (int32_t j : idx)
        if (j >= 0) out->push_back(cloud->points[j]);
    return out;
}

// ---- pcl::IterativeClosestPoint ---------------------------------------------------------------
template <class PointSource, class PointTarget>
class IterativeClosestPoint {
public:
    typedef std::array<float, 16> Matrix4;  // row-major 4x4
    void setMaximumIterations(int n) { max_iterations_ = n; }
    void setInputSource(const typename PointCloud<PointSource>::ConstPtr& c) { source_ = c; }
    void setInputTarget(const typename PointCloud<PointTarget>::ConstPtr& c) { target_ = c; tree_.setInputCloud(c); }
    // align: the ICP loop with PCL's defaults (no distance threshold, SVD/Umeyama estimate,
    // DefaultConvergenceCriteria: iteration cap or |mse - prev| < 1e-12); output = transformed source
    void align(PointCloud<PointSource>& output) {
        converged_ = false;
        final_ = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        fitness_ = DBL_MAX;
        output = *source_;
        if (!tree_.handle() || source_->empty()) return;
        int conv = 0, it = 0;
        check(pcc_icp_align(tree_.handle(), source_->points.data(), source_->size(), sizeof(PointSource), PCC_MEM_HOST,
                            max_iterations_, 0, final_.data(), &fitness_, &it, &conv));
        converged_ = conv != 0;
        iterations_ = it;
        check(pcc_transform(tree_.handle(), final_.data(), source_->points.data(), source_->size(), sizeof(PointSource),
                            output.points.data(), sizeof(PointSource), PCC_MEM_HOST));
    }
    bool hasConverged() const { return converged_; }
    double getFitnessScore() const { return fitness_; }
    Matrix4 getFinalTransformation() const { return final_; }
    int getIterations() const { return iterations_; }

private:
    int max_iterations_ = 10;  // PCL default; the reference sets 20
    int iterations_ = 0;
    bool converged_ = false;
    double fitness_ = DBL_MAX;
    Matrix4 final_{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
    typename PointCloud<PointSource>::ConstPtr source_;
    typename PointCloud<PointTarget>::ConstPtr target_;
    search::KdTree<PointTarget> tree_;
};

// ---- performICP (src/comparator.cpp:1089-1110), same printed lines ----------------------------
inline bool performICP(const PointCloud<PointXYZRGB>::Ptr& point_cloud1, const PointCloud<PointXYZRGB>::Ptr& point_cloud2) {
    IterativeClosestPoint<PointXYZRGB, PointXYZRGB> icp;
    icp.setMaximumIterations(20);
    icp.setInputSource(point_cloud1);
    icp.setInputTarget(point_cloud2);
    PointCloud<PointXYZRGB> Final;
    icp.align(Final);
    std::cout << "has converged:" << icp.hasConverged() << " ICP fitness score: " << icp.getFitnessScore() << std::endl;
    if (icp.hasConverged() == 1)
        std::cout << "ICP has converged; starting comparison of point clouds" << std::endl;
    else
        std::cout << "ICP has not converged; point clouds too much different to perform a specific comparison" << std::endl;
    return icp.hasConverged() == 1;
}

// ---- pcl::StatisticalOutlierRemoval (src/comparator.cpp:1523-1527) ---------------------------------
template <class PointT>
class StatisticalOutlierRemoval {
public:
    void setInputCloud(const typename PointCloud<PointT>::ConstPtr& c) { input_ = c; }
    void setMeanK(int k) { mean_k_ = k; }
    void setStddevMulThresh(double m) { std_mul_ = m; }
    void filter(PointCloud<PointT>& output) {
        output.points.clear();
        if (!input_ || input_->empty()) return;
        search::KdTree<PointT> tree(false);
        tree.setInputCloud(input_);
        if (!tree.handle()) return;
        std::vector<std::uint8_t> inlier(input_->size());
        size_t kept = 0;
        check(pcc_sor(tree.handle(), mean_k_, std_mul_, PCC_MEM_HOST, nullptr, inlier.data(), &threshold_, &kept));
        output.points.reserve(kept);
        for (size_t i = 0; i < input_->size(); ++i)
            if (inlier[i]) output.points.push_back(input_->points[i]);
        output.width = (std::uint32_t)output.points.size();
        output.height = 1;
    }
    double getThreshold() const { return threshold_; }

private:
    typename PointCloud<PointT>::ConstPtr input_;
    int mean_k_ = 1;
    double std_mul_ = 0.0, threshold_ = 0.0;
};

// ---- pcl::EuclideanClusterExtraction (src/segmentation.cpp:125-131) ------------------------------------
template <class PointT>
class EuclideanClusterExtraction {
public:
    void setClusterTolerance(double t) { tolerance_ = t; }
    void setMinClusterSize(int n) { min_ = n; }
    void setMaxClusterSize(int n) { max_ = n; }
    void setSearchMethod(const typename search::KdTree<PointT>::Ptr& tree) { tree_ = tree; }
    void setInputCloud(const typename PointCloud<PointT>::ConstPtr& c) { input_ = c; }
    // PCL re-runs tree_->setInputCloud(input_) inside extract; an index already
    // built on the same cloud is reused here.
    void extract(std::vector<PointIndices>& clusters) {
        clusters.clear();
        if (!input_ || input_->empty()) return;
        if (!tree_) tree_.reset(new search::KdTree<PointT>(false));
        if (!tree_->covers(input_)) tree_->setInputCloud(input_);
        if (!tree_->handle()) return;
        std::vector<int32_t> labels(input_->size());
        int32_t ncl = 0;
        check(pcc_euclidean_clusters(tree_->handle(), tolerance_, (uint32_t)min_, (uint32_t)max_, PCC_MEM_HOST,
                                     labels.data(), &ncl, nullptr, 0));
        clusters.resize(ncl);
        for (size_t i = 0; i < labels.size(); ++i)  // ascending i == PCL's sorted indices per cluster
            if (labels[i] >= 0) clusters[labels[i]].indices.push_back((int)i);
    }

private:
    double tolerance_ = 0.0;
    int min_ = 1, max_ = 0x7fffffff;
    typename search::KdTree<PointT>::Ptr tree_;
    typename PointCloud<PointT>::ConstPtr input_;
};

// ---- pcl::NormalEstimation (src/segmentation.cpp:232-241) ----------------------------------------------
template <class PointT, class NormalT = Normal>
class NormalEstimation {
public:
    void setSearchMethod(const typename search::KdTree<PointT>::Ptr& tree) { tree_ = tree; }
    void setInputCloud(const typename PointCloud<PointT>::ConstPtr& c) { input_ = c; }
    void setKSearch(int k) { k_ = k; }
    void setRadiusSearch(double r) { radius_ = r; }  // as in PCL, the radius is used when no K was set
    void setViewPoint(float x, float y, float z) { vp_[0] = x; vp_[1] = y; vp_[2] = z; }
    void compute(PointCloud<NormalT>& out) {
        out.points.clear();
        out.width = 0;
        out.height = 1;
        if (!input_ || input_->empty() || (k_ < 1 && !(radius_ > 0))) return;
        if (!tree_) tree_.reset(new search::KdTree<PointT>(false));
        if (!tree_->covers(input_)) tree_->setInputCloud(input_);
        if (!tree_->handle()) return;
        std::vector<float> nc(input_->size() * 4);
        if (k_ >= 1) check(pcc_normals(tree_->handle(), k_, vp_, PCC_MEM_HOST, nc.data()));
        else check(pcc_normals_radius(tree_->handle(), radius_, vp_, PCC_MEM_HOST, nc.data()));
        out.points.resize(input_->size());
        out.width = (std::uint32_t)input_->size();
        out.is_dense = true;
        for (size_t i = 0; i < out.points.size(); ++i) {
            NormalT& q = out.points[i];
            q.normal_x = nc[4 * i]; q.normal_y = nc[4 * i + 1]; q.normal_z = nc[4 * i + 2]; q.curvature = nc[4 * i + 3];
            if (!std::isfinite(q.normal_x)) out.is_dense = false;  // as PCL flags NaN normals
        }
    }

private:
    typename search::KdTree<PointT>::Ptr tree_;
    typename PointCloud<PointT>::ConstPtr input_;
    int k_ = 0;
    double radius_ = 0.0;
    float vp_[3] = {0.f, 0.f, 0.f};
};

// ---- pcl::RegionGrowing (src/segmentation.cpp:259-271) -------------------------------------------------
template <class PointT, class NormalT = Normal>
class RegionGrowing {
public:
    void setMinClusterSize(int n) { min_ = n; }
    void setMaxClusterSize(int n) { max_ = n; }
    void setSearchMethod(const typename search::KdTree<PointT>::Ptr& tree) { tree_ = tree; }
    void setNumberOfNeighbours(unsigned int k) { k_ = k; }
    void setInputCloud(const typename PointCloud<PointT>::ConstPtr& c) { input_ = c; }
    void setInputNormals(const typename PointCloud<NormalT>::ConstPtr& n) { normals_ = n; }
    void setSmoothnessThreshold(float theta) { theta_ = theta; }
    void setCurvatureThreshold(float c) { curvature_ = c; }
    void extract(std::vector<PointIndices>& clusters) {
        clusters.clear();
        // PCL's prepareForSegmentation: no cloud, no normals or a size mismatch -> empty result
        if (!input_ || input_->empty() || !normals_ || normals_->size() != input_->size() || k_ == 0) return;
        if (!tree_) tree_.reset(new search::KdTree<PointT>(false));
        if (!tree_->covers(input_)) tree_->setInputCloud(input_);
        if (!tree_->handle()) return;
        const size_t n = input_->size();
        std::vector<float> nc(n * 4);
        for (size_t i = 0; i < n; ++i) {
            const NormalT& q = normals_->points[i];
            nc[4 * i] = q.normal_x; nc[4 * i + 1] = q.normal_y; nc[4 * i + 2] = q.normal_z; nc[4 * i + 3] = q.curvature;
        }
        std::vector<int32_t> labels(n);
        int32_t ncl = 0;
        check(pcc_region_growing(tree_->handle(), nc.data(), PCC_MEM_HOST, (int)k_, theta_, curvature_, (uint32_t)min_,
                                 (uint32_t)max_, labels.data(), &ncl));
        clusters.resize(ncl);
        for (size_t i = 0; i < n; ++i)  // assembleRegions fills every cluster in ascending point order
            if (labels[i] >= 0) clusters[labels[i]].indices.push_back((int)i);
    }

private:
    int min_ = 1, max_ = 0x7fffffff;
    unsigned int k_ = 30;
    float theta_ = 30.0f / 180.0f * 3.14159265358979f, curvature_ = 0.05f;
    typename search::KdTree<PointT>::Ptr tree_;
    typename PointCloud<PointT>::ConstPtr input_;
    typename PointCloud<NormalT>::ConstPtr normals_;
};

// ---- pcl::SACSegmentation, plane + RANSAC (src/segmentation.cpp:79-99) --------------------------------
enum SacModel { SACMODEL_PLANE = 0 };
enum SacMethod { SAC_RANSAC = 0 };

template <class PointT>
class SACSegmentation {
public:
    void setOptimizeCoefficients(bool b) { optimize_ = b; }
    void setModelType(int m) { model_ = m; }
    void setMethodType(int m) { method_ = m; }
    void setMaxIterations(int n) { max_iterations_ = n; }
    void setDistanceThreshold(double t) { threshold_ = t; }
    void setProbability(double p) { probability_ = p; }
    void setInputCloud(const typename PointCloud<PointT>::ConstPtr& c) { input_ = c; }
    // inliers.indices empty + coefficients.values empty: no model (as PCL reports it)
    void segment(PointIndices& inliers, ModelCoefficients& coefficients) {
        inliers.indices.clear();
        coefficients.values.clear();
        if (!input_ || input_->empty()) return;
        if (model_ != SACMODEL_PLANE || method_ != SAC_RANSAC) throw Error(PCC_ERR_UNSUPPORTED, "only SACMODEL_PLANE + SAC_RANSAC");
        if (!ctx_) {
            // any index handle supplies device, stream and scratch; a one-point index is the cheapest
            const float one[3] = {0.f, 0.f, 0.f};
            check(pcc_index_create(one, 1, 12, 3, PCC_MEM_HOST, 0, PCC_ENGINE_BRUTE, &ctx_));
        }
        std::vector<int32_t> idx(input_->size());
        size_t m = 0;
        float c[4];
        check(pcc_sac_plane(ctx_, input_->points.data(), input_->size(), sizeof(PointT), PCC_MEM_HOST, max_iterations_,
                            threshold_, probability_, optimize_ ? 1 : 0, idx.data(), &m, c, nullptr));
        if (m == 0) return;
        inliers.indices.assign(idx.begin(), idx.begin() + m);
        coefficients.values.assign(c, c + 4);
    }
    SACSegmentation() = default;
    SACSegmentation(const SACSegmentation&) = delete;
    SACSegmentation& operator=(const SACSegmentation&) = delete;
    ~SACSegmentation() { if (ctx_) pcc_index_destroy(ctx_); }

private:
    bool optimize_ = false;
    int model_ = SACMODEL_PLANE, method_ = SAC_RANSAC, max_iterations_ = 50;
    double threshold_ = 0.0, probability_ = 0.99;
    typename PointCloud<PointT>::ConstPtr input_;
    pcc_index* ctx_ = nullptr;
};

// ---- pcl::ExtractIndices (src/segmentation.cpp:103-116): index bookkeeping, host only ---------------------
template <class PointT>
class ExtractIndices {
public:
    void setInputCloud(const typename PointCloud<PointT>::ConstPtr& c) { input_ = c; }
    void setIndices(const std::shared_ptr<const PointIndices>& i) { indices_ = i; }
    void setNegative(bool n) { negative_ = n; }
    void filter(PointCloud<PointT>& out) {
        std::vector<PointT> pts;
        if (input_) {
            const size_t n = input_->size();
            if (!negative_) {
                if (indices_) for (int i : indices_->indices) pts.push_back(input_->points[i]);
            } else {
                std::vector<char> drop(n, 0);
                if (indices_) for (int i : indices_->indices) drop[i] = 1;
                for (size_t i = 0; i < n; ++i) if (!drop[i]) pts.push_back(input_->points[i]);
            }
        }
        out.points.swap(pts);
        out.width = (std::uint32_t)out.points.size();
        out.height = 1;
        out.is_dense = true;
    }

private:
    typename PointCloud<PointT>::ConstPtr input_;
    std::shared_ptr<const PointIndices> indices_;
    bool negative_ = false;
};

// ---- the whole plane-removal loop (src/segmentation.cpp:79-117) in one library call ---------------------
// What the SACSegmentation::segment + ExtractIndices loop leaves: the remaining cloud (whole records, order kept) and, per
// plane removed, its inlier count and coefficients.  pcc_plane_removal uploads the cloud once and compacts it on the device.
struct RemovedPlanes {
    std::vector<std::uint32_t> sizes;                 // |cloud_plane| of every turn (:110-111)
    std::vector<std::array<float, 4> > coefficients;  // a, b, c, d of every turn
    bool ended_without_model = false;                 // the loop ended at :95-100
};
template <class PointT>
inline typename PointCloud<PointT>::Ptr removePlanes(const typename PointCloud<PointT>::ConstPtr& cloud, RemovedPlanes& planes,
                                                     double stop_fraction = 0.3, int max_iterations = 100,
                                                     double distance_threshold = 0.02, bool optimize = true,
                                                     double probability = 0.99) {
    typename PointCloud<PointT>::Ptr rest(new PointCloud<PointT>);
    planes = RemovedPlanes();
    if (!cloud || cloud->empty()) return rest;
    const float one[3] = {0.f, 0.f, 0.f};  // any index handle supplies device, stream and scratch (SACSegmentation above)
    pcc_index* ctx = nullptr;
    check(pcc_index_create(one, 1, 12, 3, PCC_MEM_HOST, 0, PCC_ENGINE_BRUTE, &ctx));
    struct Closer { pcc_index* h; ~Closer() { pcc_index_destroy(h); } } closer{ctx};
    const size_t n = cloud->size();
    rest->points.resize(n);
    size_t capacity = 64, found = 0, left = 0;
    int ended = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        planes.sizes.resize(capacity);
        planes.coefficients.resize(capacity);
        const int st = pcc_plane_removal(ctx, cloud->points.data(), n, sizeof(PointT), PCC_MEM_HOST, stop_fraction, max_iterations,
                                         distance_threshold, probability, optimize ? 1 : 0, capacity, planes.coefficients[0].data(),
                                         planes.sizes.data(), nullptr, &found, &ended, nullptr, nullptr, &left, rest->points.data(),
                                         sizeof(PointT), sizeof(PointT));
        // every plane removes at least one point: n planes always suffice
        if (st == PCC_ERR_OVERFLOW && attempt == 0) { capacity = n; continue; }
        check(st);
        break;
    }
    planes.sizes.resize(found);
    planes.coefficients.resize(found);
    planes.ended_without_model = ended != 0;
    rest->points.resize(left);
    rest->width = (std::uint32_t)left;
    rest->height = 1;
    rest->is_dense = true;
    return rest;
}

// ---- region_growing_segmentation (src/segmentation.cpp:218-327) in one library call ----------------------
// VoxelGrid leaf -> NormalEstimation normal_k -> RegionGrowing k -> one cloud per cluster: what the VoxelGrid, KdTree,
// NormalEstimation and RegionGrowing objects above give together (same filtered points, same clusters, same order), but the
// filtered cloud, its index, its normals and its labels never leave the device (pcc_region_growing_segmentation).  *filtered
// (may be null) receives the filtered cloud.  A leaf too small for the cloud (PCC_ERR_UNSUPPORTED, PCL: "leaf size is too
// small", output = input) takes the class path, as VoxelGrid::filter does.
template <class PointT>
inline std::vector<typename PointCloud<PointT>::Ptr> regionGrowingSegmentation(
    const typename PointCloud<PointT>::ConstPtr& cloud, float leaf = 0.025f, int normal_k = 50, int k = 100,
    float smoothness = (float)(3.0 / 180.0 * 3.14159265358979323846), float curvature = 1.0f, int min_size = 50, int max_size = 1000000,
    typename PointCloud<PointT>::Ptr* filtered = nullptr) {
    std::vector<typename PointCloud<PointT>::Ptr> clusters;
    typename PointCloud<PointT>::Ptr kept(new PointCloud<PointT>);
    kept->height = 1;
    kept->is_dense = true;
    if (filtered) *filtered = kept;
    if (!cloud || cloud->empty()) return clusters;
    // any index handle supplies device, stream and scratch; this one stays with the thread, and the work handle the filtered
    // cloud is indexed on stays with it
    struct Context {
        pcc_index* h = nullptr;
        ~Context() { pcc_index_destroy(h); }
    };
    static thread_local Context context;
    if (!context.h) {
        const float one[3] = {0.f, 0.f, 0.f};
        check(pcc_index_create(one, 1, 12, 3, PCC_MEM_HOST, 0, PCC_ENGINE_BRUTE, &context.h));
    }
    const size_t n = cloud->size();
    // what the call answers with PCC_ERR_UNSUPPORTED besides a leaf too small for the cloud: refused here, so that the status
    // below can only mean the leaf
    if (normal_k < 1 || normal_k > PCC_KNN_MAX_K || k < 1 || k > PCC_KNN_MAX_K)
        throw Error(PCC_ERR_UNSUPPORTED, "regionGrowingSegmentation: normal_k and k must lie in [1, PCC_KNN_MAX_K]");
    if (n >= (1ull << 31)) throw Error(PCC_ERR_UNSUPPORTED, "regionGrowingSegmentation: more than 2^31 points");
    const int has_rgb = sizeof(PointT) >= 20 ? 1 : 0;
    kept->points.resize(n);
    std::vector<PointT> members(n);
    std::vector<size_t> offsets;
    size_t capacity = 256, nv = 0;
    int32_t ncl = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        offsets.assign(capacity + 1, 0);
        const int st = pcc_region_growing_segmentation(context.h, cloud->points.data(), n, sizeof(PointT), PCC_MEM_HOST, leaf, has_rgb,
                                                       normal_k, k, smoothness, curvature, (uint32_t)min_size, (uint32_t)max_size,
                                                       kept->points.data(), sizeof(PointT), &nv, nullptr, nullptr, capacity, &ncl,
                                                       offsets.data(), members.data(), nullptr);
        if (st == PCC_ERR_OVERFLOW && attempt == 0) { capacity = (size_t)ncl; continue; }  // once more with the room it asks for
        if (st == PCC_ERR_UNSUPPORTED) {
            // (k, normal_k and n were checked above: what is left is the voxel grid's "leaf size too small")
            // the objects the call replaces, as examples/comparator_main.cpp drives them
            VoxelGrid<PointT> vg;
            vg.setInputCloud(cloud);
            vg.setLeafSize(leaf, leaf, leaf);
            vg.filter(*kept);
            typename search::KdTree<PointT>::Ptr tree(new search::KdTree<PointT>);
            tree->setOption(PCC_OPT_KNN_CACHE_K, std::max(normal_k, k));
            typename PointCloud<Normal>::Ptr normals(new PointCloud<Normal>);
            NormalEstimation<PointT, Normal> ne;
            ne.setSearchMethod(tree);
            ne.setInputCloud(kept);
            ne.setKSearch(normal_k);
            ne.compute(*normals);
            RegionGrowing<PointT, Normal> reg;
            reg.setMinClusterSize(min_size);
            reg.setMaxClusterSize(max_size);
            reg.setSearchMethod(tree);
            reg.setNumberOfNeighbours((unsigned int)k);
            reg.setInputCloud(kept);
            reg.setInputNormals(normals);
            reg.setSmoothnessThreshold(smoothness);
            reg.setCurvatureThreshold(curvature);
            std::vector<PointIndices> found;
            reg.extract(found);
            for (const PointIndices& c : found) {
                typename PointCloud<PointT>::Ptr one(new PointCloud<PointT>);
                for (int j : c.indices) one->points.push_back(kept->points[j]);
                one->width = (std::uint32_t)one->points.size();
                one->height = 1;
                one->is_dense = true;
                clusters.push_back(one);
            }
            return clusters;
        }
        check(st);
        break;
    }
    kept->points.resize(nv);
    kept->width = (std::uint32_t)nv;
    for (int32_t c = 0; c < ncl; ++c) {
        typename PointCloud<PointT>::Ptr one(new PointCloud<PointT>);
        one->points.assign(members.begin() + offsets[c], members.begin() + offsets[c + 1]);
        one->width = (std::uint32_t)one->points.size();
        one->height = 1;
        one->is_dense = true;
        clusters.push_back(one);
    }
    return clusters;
}

// ---- euclidean_cluster_segmentation (src/segmentation.cpp:64-156) in one library call ----------------------
// VoxelGrid leaf -> the plane-removal loop -> EuclideanClusterExtraction -> one cloud per cluster: what the VoxelGrid,
// SACSegmentation, ExtractIndices, KdTree and EuclideanClusterExtraction objects above give together (same planes, same
// remaining points, same clusters, same order), but the filtered cloud, what remains of it, its index and its labels never leave
// the device (pcc_euclidean_cluster_segmentation).  planes: what removePlanes reports.  *remaining (may be null) receives the cloud
// the clusters are taken from, *n_filtered (may be null) the size of the voxel grid's output.  The call starts with room for
// first_planes planes and first_clusters clusters and is repeated once with the room it asks for (tests start it with less).  A
// leaf too small for the cloud (PCC_ERR_UNSUPPORTED) takes the class path, as in regionGrowingSegmentation.
template <class PointT>
inline std::vector<typename PointCloud<PointT>::Ptr> euclideanClusterSegmentation(
    const typename PointCloud<PointT>::ConstPtr& cloud, float leaf, double stop_fraction, int max_iterations, double distance_threshold,
    bool optimize, double tolerance, int min_size, int max_size, RemovedPlanes& planes,
    typename PointCloud<PointT>::Ptr* remaining = nullptr, size_t* n_filtered = nullptr, size_t first_planes = 64,
    size_t first_clusters = 256) {
    std::vector<typename PointCloud<PointT>::Ptr> clusters;
    typename PointCloud<PointT>::Ptr rest(new PointCloud<PointT>);
    rest->height = 1;
    rest->is_dense = true;
    planes = RemovedPlanes();
    if (remaining) *remaining = rest;
    if (n_filtered) *n_filtered = 0;
    if (!cloud || cloud->empty()) return clusters;
    struct Context {
        pcc_index* h = nullptr;
        ~Context() { pcc_index_destroy(h); }
    };
    static thread_local Context context;
    if (!context.h) {
        const float one[3] = {0.f, 0.f, 0.f};
        check(pcc_index_create(one, 1, 12, 3, PCC_MEM_HOST, 0, PCC_ENGINE_BRUTE, &context.h));
    }
    const size_t n = cloud->size();
    // (the one other PCC_ERR_UNSUPPORTED of the call: refused here, so that the status below can only mean the leaf)
    if (n >= (1ull << 31)) throw Error(PCC_ERR_UNSUPPORTED, "euclideanClusterSegmentation: more than 2^31 points");
    const int has_rgb = sizeof(PointT) >= 20 ? 1 : 0;
    const double probability = 0.99;  // (SACSegmentation's default, as removePlanes)
    rest->points.resize(n);
    std::vector<PointT> members(n);
    std::vector<size_t> offsets;
    size_t plane_room = first_planes, cluster_room = first_clusters, found = 0, nv = 0, left = 0;
    int ended = 0;
    int32_t ncl = 0;
    for (int attempt = 0; attempt < 3; ++attempt) {
        planes.sizes.resize(std::max<size_t>(plane_room, 1));
        planes.coefficients.resize(std::max<size_t>(plane_room, 1));
        offsets.assign(cluster_room + 1, 0);
        const int st = pcc_euclidean_cluster_segmentation(
            context.h, cloud->points.data(), n, sizeof(PointT), PCC_MEM_HOST, leaf, has_rgb, stop_fraction, max_iterations, distance_threshold,
            probability, optimize ? 1 : 0, plane_room, planes.coefficients[0].data(), planes.sizes.data(), nullptr, &found, &ended, tolerance,
            (uint32_t)min_size, (uint32_t)max_size, rest->points.data(), sizeof(PointT), &nv, &left, nullptr, cluster_room, &ncl,
            offsets.data(), cluster_room ? members.data() : nullptr, nullptr);
        if (st == PCC_ERR_OVERFLOW && attempt < 2) {
            // once more with the room it asks for: every plane removes at least one point, so nv planes always suffice; the
            // cluster count is reported.  (Too many planes are met before any cluster: at most two repeats, one of each kind)
            if (found == plane_room && (size_t)ncl <= cluster_room) plane_room = std::max<size_t>(nv, 1);
            else cluster_room = (size_t)ncl;
            continue;
        }
        if (st == PCC_ERR_UNSUPPORTED) {
            // the objects the call replaces, as examples/comparator_main.cpp drives them
            typename PointCloud<PointT>::Ptr kept(new PointCloud<PointT>);
            VoxelGrid<PointT> vg;
            vg.setInputCloud(cloud);
            vg.setLeafSize(leaf, leaf, leaf);
            vg.filter(*kept);
            if (n_filtered) *n_filtered = kept->size();
            rest = removePlanes<PointT>(kept, planes, stop_fraction, max_iterations, distance_threshold, optimize, probability);
            if (remaining) *remaining = rest;
            typename search::KdTree<PointT>::Ptr tree(new search::KdTree<PointT>);
            tree->setInputCloud(rest);
            std::vector<PointIndices> found_clusters;
            EuclideanClusterExtraction<PointT> ec;
            ec.setClusterTolerance(tolerance);
            ec.setMinClusterSize(min_size);
            ec.setMaxClusterSize(max_size);
            ec.setSearchMethod(tree);
            ec.setInputCloud(rest);
            ec.extract(found_clusters);
            for (const PointIndices& c : found_clusters) {
                typename PointCloud<PointT>::Ptr one(new PointCloud<PointT>);
                for (int j : c.indices) one->points.push_back(rest->points[j]);
                one->width = (std::uint32_t)one->points.size();
                one->height = 1;
                one->is_dense = true;
                clusters.push_back(one);
            }
            return clusters;
        }
        check(st);
        break;
    }
    planes.sizes.resize(found);
    planes.coefficients.resize(found);
    planes.ended_without_model = ended != 0;
    if (n_filtered) *n_filtered = nv;
    rest->points.resize(left);
    rest->width = (std::uint32_t)left;
    for (int32_t c = 0; c < ncl; ++c) {
        typename PointCloud<PointT>::Ptr one(new PointCloud<PointT>);
        one->points.assign(members.begin() + offsets[c], members.begin() + offsets[c + 1]);
        one->width = (std::uint32_t)one->points.size();
        one->height = 1;
        one->is_dense = true;
        clusters.push_back(one);
    }
    return clusters;
}

}  // namespace pcc
