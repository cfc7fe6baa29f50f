// region_growing_rgb.hpp -- pcl::RegionGrowingRGB as the reference uses it in color_growing_segmentation
// (src/segmentation.cpp:161-216: distance threshold 10, point colour threshold 6, region colour threshold 5, minimum
// cluster size 200; called twice per accepted match, src/comparator.cpp:1466-1500, where only the NUMBER of colour
// segments enters the report).
//
// Where the time goes in PCL: findPointNeighbours() -- one nearestKSearch with 100 neighbours per point.  That is the
// part this repository accelerates: ONE batched self k-NN on the GPU (pcc_knn, rows ascending by (d2, index)).  What PCL
// does with the rows is sequential, order-dependent host logic and stays host logic here, statement for statement in
// PCL's order (restated from PCL 1.7's region_growing.hpp / region_growing_rgb.hpp -- SURVEY.md 9 has no section for
// it; the same recollection, written independently in C, is the test oracle's restatement):
//   1. growing: seeds in index order, breadth first over the first `neighbour_number_` (30) neighbours of a point, a
//      neighbour joins when its squared colour distance to the CURRENT point is <= point threshold^2; every joined point
//      spreads (no normals, no curvature test in this configuration);
//   2. segment neighbours: per segment the `region_neighbour_number_` (100) nearest other segments, by the smallest
//      neighbour distance over its points' rows;
//   3. merging: segments whose MEAN colours (float sums in index order, truncated to integers) differ by less than
//      region threshold^2 and that lie within distance threshold^2 join a homogeneous region; regions below the minimum
//      size are folded into their nearest neighbouring region;
//   4. clusters outside [min, max] size are dropped.
// PCL orders a region's neighbour list with std::sort, which leaves the order of equal distances unspecified; this mirror
// (and the oracle) use a stable sort -- one of the orders PCL may produce.
//
// setDeviceSegmentation(true) hands ALL of it to the library instead: extract() is then one pcc_region_growing_rgb call (rows,
// growing, segment statistics and segment pairs on the GPU, the merging on the host inside the library, labels back) -- the
// same clusters, bit for bit; nothing but the labels crosses to this side.  Off by default: extract() above is untouched.
//
// color_growing_segmentation_batch does the same for MANY clouds in one pcc_region_growing_rgb_batch call -- the two
// segmentations of every accepted match of a comparison, none of which depends on another.
//
// matchColourElements goes one step further for the match loop (src/comparator.cpp:1379-1509), which keeps only the NUMBER of
// colour segments of either cluster: the clusters of both scenes and the match table in ONE pcc_match_colour_elements call, every
// distinct cluster segmented once, nothing but the counts coming back.
#pragma once
#include <algorithm>
#include <array>
#include <limits>
#include <queue>
#include <stdexcept>
#include <utility>
#include <vector>
#include "pcc/search.hpp"

namespace pcc {

template <class PointT>
class RegionGrowingRGB {
public:
    typedef typename PointCloud<PointT>::ConstPtr CloudConstPtr;
    typedef typename search::KdTree<PointT>::Ptr KdTreePtr;
    void setInputCloud(const CloudConstPtr& c) { input_ = c; }
    void setSearchMethod(const KdTreePtr& t) { search_ = t; }
    void setDistanceThreshold(float t) { distance_threshold_ = t * t; distance_given_ = t; }
    void setPointColorThreshold(float t) { color_p2p_threshold_ = t * t; color_p2p_given_ = t; }
    void setRegionColorThreshold(float t) { color_r2r_threshold_ = t * t; color_r2r_given_ = t; color_r2r_set_ = true; }
    void setMinClusterSize(int n) { min_pts_per_cluster_ = n; }
    void setMaxClusterSize(int n) { max_pts_per_cluster_ = n; }
    void setNumberOfNeighbours(unsigned int k) { neighbour_number_ = k; }
    void setNumberOfRegionNeighbours(unsigned int k) { region_neighbour_number_ = k; }
    // (not in PCL) true: extract() is one pcc_region_growing_rgb call on the search method's handle
    void setDeviceSegmentation(bool on) { device_segmentation_ = on; }
    bool getDeviceSegmentation() const { return device_segmentation_; }

    void extract(std::vector<PointIndices>& clusters) {
        clusters.clear();
        if (!input_ || input_->empty()) return;
        if (region_neighbour_number_ == 0 || neighbour_number_ == 0 || color_p2p_threshold_ < 0.f || color_r2r_threshold_ < 0.f ||
            distance_threshold_ < 0.f)
            return;
        if (!search_) search_.reset(new search::KdTree<PointT>);
        search_->setInputCloud(input_);
        n_ = input_->size();
        if (device_segmentation_) { extractOnDevice(clusters); return; }
        findPointNeighbours();
        growSegments();
        findSegmentNeighbours();
        mergeRegions();
        for (const PointIndices& c : clusters_)
            if ((int)c.indices.size() >= min_pts_per_cluster_ && (int)c.indices.size() <= max_pts_per_cluster_) clusters.push_back(c);
    }

private:
    // the whole of extract() in the library: labels[i] = cluster of point i in PCL's output order, or -1
    void extractOnDevice(std::vector<PointIndices>& clusters) {
        if (!search_->handle()) return;  // no finite point: PCL's "empty input cloud"
        // PCL's default region colour threshold is 10 SQUARED, which has no float root to hand to the library: the two paths
        // would merge differently, so the device path asks for the threshold to be set (color_growing_segmentation does)
        if (!color_r2r_set_) throw std::invalid_argument("pcc::RegionGrowingRGB: setRegionColorThreshold before extract() with setDeviceSegmentation(true)");
        std::vector<int32_t> labels(n_, -1);
        int32_t ncl = 0;
        check(pcc_region_growing_rgb(search_->handle(), &input_->points[0].rgba, sizeof(PointT), PCC_MEM_HOST, distance_given_, color_p2p_given_,
                                     color_r2r_given_, (uint32_t)std::max(min_pts_per_cluster_, 0), (uint32_t)std::max(max_pts_per_cluster_, 0),
                                     neighbour_number_, region_neighbour_number_, labels.data(), &ncl));
        clusters.resize((size_t)ncl);
        for (size_t i = 0; i < n_; ++i)
            if (labels[i] >= 0) clusters[(size_t)labels[i]].indices.push_back((int)i);
    }
    // rows of the self k-NN: row_len_ entries per point, ascending by (d2, index) -- the one GPU call of this class
    void findPointNeighbours() {
        row_len_ = (int)std::min<size_t>(region_neighbour_number_, n_);
        search_->nearestKSearchBatch(*input_, row_len_, nbr_, nbr_d2_);
        // (rows of non-finite points hold -1: color_growing_segmentation strips NaNs first, PCL would assert on them)
    }
    static unsigned int colourDiff(const PointT& a, const PointT& b) {
        const int dr = (int)a.r - (int)b.r, dg = (int)a.g - (int)b.g, db = (int)a.b - (int)b.b;
        return (unsigned int)(dr * dr + dg * dg + db * db);
    }
    void growSegments() {
        label_.assign(n_, -1);
        seg_size_.clear();
        size_t seed = 0;
        size_t done = 0;
        while (done < n_) {
            while (label_[seed] != -1) ++seed;  // the next unlabelled point in index order
            const int seg = (int)seg_size_.size();
            std::queue<int> q;
            q.push((int)seed);
            label_[seed] = seg;
            int count = 1;
            while (!q.empty()) {
                const int cur = q.front();
                q.pop();
                const int* row = nbr_.data() + (size_t)cur * row_len_;
                for (unsigned int j = 0; j < neighbour_number_ && j < (unsigned int)row_len_; ++j) {
                    const int v = row[j];
                    if (v < 0 || label_[(size_t)v] != -1) continue;
                    if ((float)colourDiff(input_->points[(size_t)cur], input_->points[(size_t)v]) > color_p2p_threshold_) continue;
                    label_[(size_t)v] = seg;
                    ++count;
                    q.push(v);
                }
            }
            seg_size_.push_back(count);
            done += (size_t)count;
        }
    }
    void findSegmentNeighbours() {
        const size_t ns = seg_size_.size();
        std::vector<std::vector<int> > members(ns);
        for (size_t s = 0; s < ns; ++s) members[s].reserve((size_t)seg_size_[s]);
        for (size_t i = 0; i < n_; ++i) members[(size_t)label_[i]].push_back((int)i);
        seg_nbr_.assign(ns, std::vector<int>());
        seg_dist_.assign(ns, std::vector<float>());
        const float fmax = std::numeric_limits<float>::max();
        std::vector<float> best(ns, fmax);
        std::vector<int> touched;
        for (size_t s = 0; s < ns; ++s) {
            touched.clear();
            for (int p : members[s]) {
                const int* row = nbr_.data() + (size_t)p * row_len_;
                const float* rd = nbr_d2_.data() + (size_t)p * row_len_;
                for (int j = 0; j < row_len_; ++j) {
                    if (row[j] < 0) continue;
                    const int t = label_[(size_t)row[j]];
                    if (t == (int)s) continue;
                    if (best[(size_t)t] == fmax) touched.push_back(t);
                    if (best[(size_t)t] > rd[j]) best[(size_t)t] = rd[j];
                }
            }
            // the region_neighbour_number_ nearest, handed over farthest first (PCL pops a max-heap of (distance, segment))
            std::sort(touched.begin(), touched.end());
            std::priority_queue<std::pair<float, int> > heap;
            for (int t : touched) {
                heap.push(std::make_pair(best[(size_t)t], t));
                if (heap.size() > region_neighbour_number_) heap.pop();
                best[(size_t)t] = fmax;
            }
            while (!heap.empty()) {
                seg_dist_[s].push_back(heap.top().first);
                seg_nbr_[s].push_back(heap.top().second);
                heap.pop();
            }
        }
    }
    static bool lessFirst(const std::pair<float, int>& a, const std::pair<float, int>& b) { return a.first < b.first; }
    void mergeRegions() {
        const size_t ns = seg_size_.size();
        const float fmax = std::numeric_limits<float>::max();
        // mean colour per segment as PCL's applyRegionMergingAlgorithm takes it: the channel sums in std::vector<unsigned int>
        // (EXACT -- a float sum rounds from 2^24 on, i.e. from ~66k bright points per segment, and the truncated mean can
        // then be off by one and flip a merge), then float(sum) / float(count) truncated to an unsigned integer
        std::vector<unsigned int> sum(ns * 3, 0u);
        for (size_t i = 0; i < n_; ++i) {
            const PointT& p = input_->points[i];
            unsigned int* c = &sum[(size_t)label_[i] * 3];
            c[0] += p.r; c[1] += p.g; c[2] += p.b;
        }
        std::vector<float> col(ns * 3, 0.f);
        for (size_t s = 0; s < ns; ++s)
            for (int a = 0; a < 3; ++a)
                col[s * 3 + a] = (float)static_cast<unsigned int>(static_cast<float>(sum[s * 3 + a]) / static_cast<float>(seg_size_[s]));
        std::vector<int> seg_region(ns, -1);
        std::vector<unsigned int> reg_pts;
        std::vector<int> reg_segs;
        for (size_t s = 0; s < ns; ++s) {
            int cur;
            if (seg_region[s] == -1) {
                cur = (int)reg_pts.size();
                seg_region[s] = cur;
                reg_pts.push_back((unsigned int)seg_size_[s]);
                reg_segs.push_back(1);
            } else {
                cur = seg_region[s];
            }
            for (size_t j = 0; j < region_neighbour_number_ && j < seg_nbr_[s].size(); ++j) {
                const int t = seg_nbr_[s][j];
                if (seg_dist_[s][j] > distance_threshold_) continue;
                if (seg_region[(size_t)t] != -1) continue;
                float diff = 0.f;
                for (int a = 0; a < 3; ++a) {
                    const float d = col[s * 3 + a] - col[(size_t)t * 3 + a];
                    diff += d * d;
                }
                if (diff < color_r2r_threshold_) {
                    seg_region[(size_t)t] = cur;
                    reg_pts[(size_t)cur] += (unsigned int)seg_size_[(size_t)t];
                    reg_segs[(size_t)cur] += 1;
                }
            }
        }
        const size_t nr = reg_pts.size();
        std::vector<std::vector<int> > reg_members(nr);
        for (size_t s = 0; s < ns; ++s) reg_members[(size_t)seg_region[s]].push_back((int)s);
        // neighbours of every region: the neighbour entries of its segments that lead out of it, nearest first
        std::vector<std::vector<std::pair<float, int> > > reg_nbr(nr);
        for (size_t r = 0; r < nr; ++r) {
            for (int s : reg_members[r])
                for (size_t j = 0; j < seg_nbr_[(size_t)s].size(); ++j) {
                    if (seg_dist_[(size_t)s][j] == fmax) continue;
                    const int t = seg_nbr_[(size_t)s][j];
                    if (seg_region[(size_t)t] != (int)r) reg_nbr[r].push_back(std::make_pair(seg_dist_[(size_t)s][j], t));
                }
            std::stable_sort(reg_nbr[r].begin(), reg_nbr[r].end(), lessFirst);
        }
        // regions below the minimum size fold into the region of their nearest neighbouring segment
        for (size_t r = 0; r < nr; ++r) {
            if (reg_pts[r] >= (unsigned int)min_pts_per_cluster_) continue;
            if (reg_nbr[r].empty() || reg_nbr[r][0].first == fmax) continue;
            const int into = seg_region[(size_t)reg_nbr[r][0].second];
            const std::vector<int> moved = reg_members[r];
            for (int s : moved) {
                reg_members[(size_t)into].push_back(s);
                seg_region[(size_t)s] = into;
            }
            reg_members[r].clear();
            reg_pts[(size_t)into] += reg_pts[r];
            reg_pts[r] = 0;
            reg_segs[(size_t)into] += reg_segs[r];
            reg_segs[r] = 0;
            for (std::pair<float, int>& e : reg_nbr[(size_t)into])
                if (seg_region[(size_t)e.second] == into) { e.first = fmax; e.second = 0; }
            for (const std::pair<float, int>& e : reg_nbr[r])
                if (seg_region[(size_t)e.second] != into) reg_nbr[(size_t)into].push_back(e);
            reg_nbr[r].clear();
            std::stable_sort(reg_nbr[(size_t)into].begin(), reg_nbr[(size_t)into].end(), lessFirst);
        }
        // the regions as clusters, members in index order; empty regions dropped
        std::vector<PointIndices> all(nr);
        for (size_t r = 0; r < nr; ++r) all[r].indices.reserve(reg_pts[r]);
        for (size_t i = 0; i < n_; ++i) all[(size_t)seg_region[(size_t)label_[i]]].indices.push_back((int)i);
        clusters_.clear();
        for (PointIndices& c : all)
            if (!c.indices.empty()) clusters_.push_back(c);
    }

    CloudConstPtr input_;
    KdTreePtr search_;
    size_t n_ = 0;
    int row_len_ = 0;
    float distance_threshold_ = 0.05f * 0.05f, color_p2p_threshold_ = 1225.0f, color_r2r_threshold_ = 10.0f;
    // the thresholds as given, for the device path, which squares them itself (0.05f and 35.0f square to the defaults above)
    float distance_given_ = 0.05f, color_p2p_given_ = 35.0f, color_r2r_given_ = 0.0f;
    bool color_r2r_set_ = false;
    bool device_segmentation_ = false;
    unsigned int neighbour_number_ = 30, region_neighbour_number_ = 100;
    int min_pts_per_cluster_ = 10, max_pts_per_cluster_ = std::numeric_limits<int>::max();
    std::vector<int> nbr_, label_, seg_size_;
    std::vector<float> nbr_d2_;
    std::vector<std::vector<int> > seg_nbr_;
    std::vector<std::vector<float> > seg_dist_;
    std::vector<PointIndices> clusters_;
};

// color_growing_segmentation (reference src/segmentation.cpp:161-216) -- the number of colour segments is what the report
// uses; the segments themselves are returned as the reference returns them
template <class PointT>
inline std::vector<typename PointCloud<PointT>::Ptr> color_growing_segmentation(const typename PointCloud<PointT>::Ptr& cloud_in,
                                                                                bool device_segmentation = false) {
    std::vector<typename PointCloud<PointT>::Ptr> out;
    typename PointCloud<PointT>::Ptr cloud(new PointCloud<PointT>);
    for (const PointT& p : cloud_in->points)  // pcl::removeNaNFromPointCloud
        if (isFinite(p)) cloud->push_back(p);
    if (cloud->size() <= 10) return out;
    RegionGrowingRGB<PointT> reg;
    reg.setInputCloud(cloud);
    reg.setDistanceThreshold(10);
    reg.setPointColorThreshold(6);
    reg.setRegionColorThreshold(5);
    reg.setMinClusterSize(200);
    reg.setDeviceSegmentation(device_segmentation);
    std::vector<PointIndices> clusters;
    reg.extract(clusters);
    for (const PointIndices& c : clusters) {
        typename PointCloud<PointT>::Ptr seg(new PointCloud<PointT>);
        for (int i : c.indices) seg->push_back(cloud->points[(size_t)i]);
        out.push_back(seg);
    }
    return out;
}

// the same with the segmentation on the device (pcc_region_growing_rgb): the same gate of more than 10 points, the same NaN
// strip, the same segments
template <class PointT>
inline std::vector<typename PointCloud<PointT>::Ptr> color_growing_segmentation_device(const typename PointCloud<PointT>::Ptr& cloud_in) {
    return color_growing_segmentation<PointT>(cloud_in, true);
}

namespace detail {
// One pcc_region_growing_rgb_batch call over `clouds` (null or empty ones are empty clouds of the batch): the labels of cloud c
// are labels[offsets[c] .. offsets[c + 1]), its cluster count n_clusters[c].  ctx (nullable): any handle to lend device, stream
// and scratch.  No cloud with a point: no library call.
template <class PointT>
inline void rgbBatchCall(const std::vector<typename PointCloud<PointT>::Ptr>& clouds, float distance_threshold, float point_color_threshold,
                         float region_color_threshold, int min_cluster_size, pcc_index* ctx, std::vector<int32_t>& labels,
                         std::vector<size_t>& offsets, std::vector<int32_t>& n_clusters) {
    const size_t nc = clouds.size();
    const BatchClouds b(clouds);
    offsets = b.offsets;
    n_clusters.assign(nc, 0);
    labels.assign(offsets[nc], -1);
    if (offsets[nc] == 0) return;
    // (PCL's defaults of 30 growing and 100 region neighbours, no upper size limit: what RegionGrowingRGB above starts with)
    check(pcc_region_growing_rgb_batch(batchContext<PointT>(ctx), nc, b.pts.data(), b.n.data(), sizeof(PointT), b.rgb.data(), sizeof(PointT), PCC_MEM_HOST,
                                       distance_threshold, point_color_threshold, region_color_threshold,
                                       (uint32_t)std::max(min_cluster_size, 0), (uint32_t)std::numeric_limits<int>::max(), 30u, 100u,
                                       labels.data(), n_clusters.data()));
}
}  // namespace detail

// color_growing_segmentation for every cloud of `clouds` in ONE library call: element c of the result is what
// color_growing_segmentation(clouds[c]) returns -- the same NaN strip, the same gate of more than 10 points (a cloud at or below
// it is not sent and yields an empty list), the same segments in the same order.
template <class PointT>
inline std::vector<std::vector<typename PointCloud<PointT>::Ptr> > color_growing_segmentation_batch(
    const std::vector<typename PointCloud<PointT>::Ptr>& clouds, pcc_index* ctx = nullptr) {
    typedef typename PointCloud<PointT>::Ptr Ptr;
    std::vector<std::vector<Ptr> > out(clouds.size());
    std::vector<Ptr> sent(clouds.size());
    for (size_t c = 0; c < clouds.size(); ++c) {
        if (!clouds[c]) continue;
        Ptr cloud(new PointCloud<PointT>);
        for (const PointT& p : clouds[c]->points)  // pcl::removeNaNFromPointCloud
            if (isFinite(p)) cloud->push_back(p);
        if (cloud->size() > 10) sent[c] = cloud;
    }
    std::vector<int32_t> labels, n_clusters;
    std::vector<size_t> offsets;
    detail::rgbBatchCall<PointT>(sent, 10.f, 6.f, 5.f, 200, ctx, labels, offsets, n_clusters);
    for (size_t c = 0; c < clouds.size(); ++c) {
        if (!sent[c]) continue;
        out[c].resize((size_t)n_clusters[c]);
        for (Ptr& seg : out[c]) seg.reset(new PointCloud<PointT>);
        const int32_t* l = labels.data() + offsets[c];
        for (size_t i = 0; i < sent[c]->size(); ++i)
            if (l[i] >= 0) out[c][(size_t)l[i]]->push_back(sent[c]->points[i]);
    }
    return out;
}

// The colour-element counts of the match loop in ONE library call (pcc_match_colour_elements): element i is {-1, -1} when
// matches[i] == -1, else {color_growing_segmentation(clusters1[i]).size(), color_growing_segmentation(clusters2[matches[i]]).size()}
// -- the same gate of more than 10 finite points, the reference's thresholds 10 / 6 / 5, minimum cluster size 200, PCL's 30 and
// 100 neighbours.  The clusters of a scene (null: an empty one) are concatenated once into one record array with offsets; a
// cluster of scene 2 that several matches name is segmented once.  ctx (nullable): any handle to lend device, stream and scratch.
// No match at all: no library call.
inline std::vector<std::array<int, 2> > matchColourElements(const std::vector<PointCloud<PointXYZRGB>::Ptr>& clusters1,
                                                            const std::vector<PointCloud<PointXYZRGB>::Ptr>& clusters2,
                                                            const std::vector<int>& matches, pcc_index* ctx = nullptr) {
    const size_t nc1 = clusters1.size(), nc2 = clusters2.size();
    if (matches.size() != nc1) throw Error(PCC_ERR_INVALID, "matchColourElements: one match per cluster of the first scene");
    std::vector<std::array<int, 2> > out(nc1, std::array<int, 2>{{-1, -1}});
    if (std::all_of(matches.begin(), matches.end(), [](int m) { return m == -1; })) return out;
    std::vector<PointXYZRGB> all[2];
    std::vector<size_t> offsets[2];
    for (int s = 0; s < 2; ++s) {
        const std::vector<PointCloud<PointXYZRGB>::Ptr>& clusters = s ? clusters2 : clusters1;
        offsets[s].assign(clusters.size() + 1, 0);
        for (size_t c = 0; c < clusters.size(); ++c) offsets[s][c + 1] = offsets[s][c] + (clusters[c] ? clusters[c]->size() : 0);
        all[s].reserve(offsets[s].back());
        for (size_t c = 0; c < clusters.size(); ++c)
            if (clusters[c]) all[s].insert(all[s].end(), clusters[c]->points.begin(), clusters[c]->points.end());
    }
    const std::vector<int32_t> table(matches.begin(), matches.end());
    static_assert(sizeof(std::array<int, 2>) == 2 * sizeof(int32_t), "rows of two");
    const void* pts[2] = {all[0].empty() ? nullptr : &all[0][0].x, all[1].empty() ? nullptr : &all[1][0].x};
    const void* rgb[2] = {all[0].empty() ? nullptr : &all[0][0].rgba, all[1].empty() ? nullptr : &all[1][0].rgba};
    check(pcc_match_colour_elements(detail::batchContext<PointXYZRGB>(ctx), pts[0], rgb[0], offsets[0].data(), nc1, pts[1], rgb[1], offsets[1].data(), nc2,
                                    sizeof(PointXYZRGB), sizeof(PointXYZRGB), PCC_MEM_HOST, table.data(), 10, 10.f, 6.f, 5.f, 200u,
                                    (uint32_t)std::numeric_limits<int>::max(), 30u, 100u, out[0].data()));
    return out;
}

}  // namespace pcc
