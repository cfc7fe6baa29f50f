// fpfh.hpp -- pcc::processFPFH: the reference's processFPFH (src/comparator.cpp:824-875) re-hosted on libpcc_nn.
// Same signature, radii (normals 0.03, FPFH 0.05) and bins (11 + 11 + 11) as the reference; the whole pipeline -- normals,
// removal of NaN normals, the SPFH signatures and their weighted sums -- is one pcc_fpfh_descriptors call on a tree over the
// cloud.  It prints the two lines the reference prints.
// pcc::matchFPFH: the reference's matchFPFH (:877-910), a k = 1 search on the 33 bins, and pcc::matchFPFHBatch for many pairs: one
// pcc_match_fpfh_batch call either way.
#pragma once
#include <cmath>
#include <iostream>
#include <utility>
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

// processFPFH for every cloud of `clouds` in ONE library call (pcc_fpfh_descriptors_batch): element c of the result is what
// processFPFH(clouds[c]) returns, bit for bit (a null or empty cloud, or one without a finite point, gives empty descriptors).
// The clouds are laid one behind the other for the call.  It prints nothing.
// point_indices (nullable): per cloud, the index in that cloud of the point every returned descriptor belongs to.
// ctx (nullable): any tree whose handle may serve as the call's context; the cloud it indexes is not read.
inline std::vector<PointCloud<FPFHSignature33>::Ptr> processFPFHBatch(const std::vector<PointCloud<PointXYZRGB>::Ptr>& clouds,
                                                                      search::KdTree<PointXYZRGB>* ctx = nullptr,
                                                                      std::vector<std::vector<int> >* point_indices = nullptr) {
    std::vector<PointCloud<FPFHSignature33>::Ptr> result(clouds.size());
    for (PointCloud<FPFHSignature33>::Ptr& d : result) {
        d.reset(new PointCloud<FPFHSignature33>);
        d->width = 0;
        d->height = 1;
        d->is_dense = true;
    }
    if (point_indices) point_indices->assign(clouds.size(), std::vector<int>());
    std::vector<size_t> offsets(clouds.size() + 1, 0);
    for (size_t c = 0; c < clouds.size(); ++c) offsets[c + 1] = offsets[c] + (clouds[c] ? clouds[c]->size() : 0);
    const size_t total = offsets.back();
    if (total == 0) return result;  // (no library call)
    std::vector<PointXYZRGB> all;
    all.reserve(total);
    for (size_t c = 0; c < clouds.size(); ++c)
        if (clouds[c]) all.insert(all.end(), clouds[c]->points.begin(), clouds[c]->points.end());
    std::vector<size_t> out_offsets(clouds.size() + 1, 0);
    std::vector<FPFHSignature33> hist(total);
    std::vector<int32_t> index(total);
    check(pcc_fpfh_descriptors_batch(detail::batchContext<PointXYZRGB>(ctx ? ctx->handle() : nullptr), &all[0].x, sizeof(PointXYZRGB), offsets.data(),
                                     clouds.size(), PCC_MEM_HOST, 0.03, 0.05, 11, 11, 11, hist[0].histogram, index.data(), out_offsets.data()));
    for (size_t c = 0; c < clouds.size(); ++c) {
        PointCloud<FPFHSignature33>& d = *result[c];
        d.points.assign(hist.begin() + out_offsets[c], hist.begin() + out_offsets[c + 1]);
        d.width = (std::uint32_t)d.points.size();
        if (point_indices) (*point_indices)[c].assign(index.begin() + out_offsets[c], index.begin() + out_offsets[c + 1]);
    }
    return result;
}

// ---- matchFPFH (src/comparator.cpp:877-910) for many pairs at once ---------------------------------------------------------------
// pairs[p] = (descriptors1, descriptors2); element p of the result is the dummy 0 (:889), then per element of descriptors2 in order
// the index of its nearest element of descriptors1 when the squared distance over the 33 bins is < threshold (:901).  A
// descriptor with a non-finite bin is never returned and finds nothing; among descriptors at exactly the same distance the lowest
// index is named.  A null or empty cloud on either side gives the dummy alone.  One pcc_match_fpfh_batch: one upload, one search
// launch and one wait for all pairs; no pair at all makes no library call.  ctx (nullable) lends device, stream and scratch.
inline std::vector<std::vector<int> > matchFPFHBatch(
    const std::vector<std::pair<PointCloud<FPFHSignature33>::Ptr, PointCloud<FPFHSignature33>::Ptr> >& pairs, float threshold = 0.25f,
    search::KdTree<PointXYZRGB>* ctx = nullptr) {
    std::vector<std::vector<int> > result(pairs.size(), std::vector<int>(1));
    if (pairs.empty()) return result;
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
    check(pcc_match_fpfh_batch(detail::batchContext<PointXYZRGB>(ctx ? ctx->handle() : nullptr), pairs.size(), d1.data(), n1.data(), d2.data(),
                               n2.data(), sizeof(FPFHSignature33), PCC_MEM_HOST, threshold, out.data(), nullptr, offsets.data()));
    for (size_t p = 0; p < pairs.size(); ++p) result[p].assign(out.begin() + offsets[p], out.begin() + offsets[p + 1]);
    return result;
}

// The reference's signature and its leading 0, threshold 0.25f; it prints the reference's line per element of descriptors2 whose
// histogram[0] is not finite (:895, :906).
inline std::vector<int> matchFPFH(const PointCloud<FPFHSignature33>::Ptr& descriptors1, const PointCloud<FPFHSignature33>::Ptr& descriptors2,
                                  search::KdTree<PointXYZRGB>* ctx = nullptr) {
    if (descriptors2)
        for (const FPFHSignature33& d : descriptors2->points)
            if (!std::isfinite(d.histogram[0])) std::cout << "Found NaN in FPFH descriptors" << std::endl;
    return matchFPFHBatch(std::vector<std::pair<PointCloud<FPFHSignature33>::Ptr, PointCloud<FPFHSignature33>::Ptr> >(
                              1, std::make_pair(descriptors1, descriptors2)), 0.25f, ctx)[0];
}

}  // namespace pcc
