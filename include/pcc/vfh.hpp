// vfh.hpp -- pcc::processVHF and pcc::matchVHF: the reference's processVHF (src/comparator.cpp:482-516) and matchVHF (:471-480)
// re-hosted on libpcc_nn.  Same signatures and settings as the reference (normals at 0.03, setNormalizeBins(true),
// setNormalizeDistance(false)); the whole pipeline -- normals, the two centroids, one vote per point, the 308 bins -- is one
// pcc_vfh_descriptor call on a tree over the cloud, the distance one pcc_match_vfh call.  Like the reference's they print nothing.
// pcc::processVHFBatch is processVHF for every cluster of a comparison in ONE pcc_vfh_descriptors_batch call, and the matrix
// overload of matchVHF every distance between two such results in ONE pcc_match_vfh call.
#pragma once
#include <vector>

#include "pcc/search.hpp"

namespace pcc {

// One descriptor for the whole cloud; none (an empty cloud, as PCL leaves it when initCompute fails) for a null cloud or one of
// fewer than 2 points.  A cloud with a non-finite point throws pcc::Error (PCC_ERR_UNSUPPORTED): the reference strips such
// points when it loads a cloud (:1144-1148).
inline PointCloud<VFHSignature308>::Ptr processVHF(const PointCloud<PointXYZRGB>::Ptr& cloud, search::KdTree<PointXYZRGB>* tree = nullptr) {
    PointCloud<VFHSignature308>::Ptr descriptor(new PointCloud<VFHSignature308>);
    size_t n_out = 0;
    search::KdTree<PointXYZRGB> local;
    VFHSignature308 d;
    if (cloud && cloud->size() >= 2) {
        if (!tree) { local.setInputCloud(cloud); tree = &local; }
        if (!tree->handle()) throw Error(PCC_ERR_UNSUPPORTED, "VFH of a cloud without a finite point");
        check(pcc_vfh_descriptor(tree->handle(), PCC_MEM_HOST, 0.03, d.histogram, &n_out));
    }
    if (n_out) descriptor->points.push_back(d);
    descriptor->width = (std::uint32_t)n_out;
    descriptor->height = 1;
    descriptor->is_dense = true;
    return descriptor;
}

// The reference's signature: the distance between element 0 of either cloud (it calls at(0), which throws on an empty cloud;
// so does this).  ctx (nullable): any tree whose handle may serve as the call's context; the cloud it indexes is not read.
inline double matchVHF(const PointCloud<VFHSignature308>::Ptr& vhf1, const PointCloud<VFHSignature308>::Ptr& vhf2,
                       search::KdTree<PointXYZRGB>* ctx = nullptr) {
    const VFHSignature308 &a = vhf1->points.at(0), &b = vhf2->points.at(0);
    double dis = 0;
    check(pcc_match_vfh(detail::batchContext<PointXYZRGB>(ctx ? ctx->handle() : nullptr), a.histogram, 1, b.histogram, 1, PCC_MEM_HOST, &dis));
    return dis;
}

// processVHF for every cloud of `clouds` in ONE library call (pcc_vfh_descriptors_batch): element c of the result is what
// processVHF(clouds[c]) returns, bit for bit; a null cloud, or one of fewer than 2 points, gives an empty descriptor cloud.
// The clouds are laid one behind the other for the call.  A cloud of 2 points and more with a non-finite point throws pcc::Error
// (PCC_ERR_UNSUPPORTED).  It prints nothing.
// ctx (nullable): any tree whose handle may serve as the call's context; the cloud it indexes is not read.
inline std::vector<PointCloud<VFHSignature308>::Ptr> processVHFBatch(const std::vector<PointCloud<PointXYZRGB>::Ptr>& clouds,
                                                                     search::KdTree<PointXYZRGB>* ctx = nullptr) {
    std::vector<PointCloud<VFHSignature308>::Ptr> result(clouds.size());
    for (PointCloud<VFHSignature308>::Ptr& d : result) {
        d.reset(new PointCloud<VFHSignature308>);
        d->width = 0;
        d->height = 1;
        d->is_dense = true;
    }
    std::vector<size_t> offsets(clouds.size() + 1, 0);
    size_t rows = 0;
    for (size_t c = 0; c < clouds.size(); ++c) {
        const size_t n = clouds[c] ? clouds[c]->size() : 0;
        offsets[c + 1] = offsets[c] + n;
        rows += n >= 2 ? 1 : 0;
    }
    if (rows == 0) return result;  // (no library call)
    std::vector<PointXYZRGB> all;
    all.reserve(offsets.back());
    for (size_t c = 0; c < clouds.size(); ++c)
        if (clouds[c]) all.insert(all.end(), clouds[c]->points.begin(), clouds[c]->points.end());
    std::vector<size_t> out_offsets(clouds.size() + 1, 0);
    std::vector<VFHSignature308> hist(rows);
    check(pcc_vfh_descriptors_batch(detail::batchContext<PointXYZRGB>(ctx ? ctx->handle() : nullptr), &all[0].x, sizeof(PointXYZRGB), offsets.data(),
                                    clouds.size(), PCC_MEM_HOST, 0.03, hist[0].histogram, out_offsets.data()));
    for (size_t c = 0; c < clouds.size(); ++c) {
        PointCloud<VFHSignature308>& d = *result[c];
        d.points.assign(hist.begin() + out_offsets[c], hist.begin() + out_offsets[c + 1]);
        d.width = (std::uint32_t)d.points.size();
    }
    return result;
}

// matchVHF for every pair of two lists of descriptor clouds (what processVHFBatch returns) in ONE pcc_match_vfh call: the
// row-major n1 x n2 distances between element 0 of the non-empty clouds of d1 and of d2, in their order; null and empty clouds
// are passed over.
inline std::vector<double> matchVHF(const std::vector<PointCloud<VFHSignature308>::Ptr>& d1,
                                    const std::vector<PointCloud<VFHSignature308>::Ptr>& d2, search::KdTree<PointXYZRGB>* ctx = nullptr) {
    std::vector<VFHSignature308> a, b;
    for (const PointCloud<VFHSignature308>::Ptr& d : d1)
        if (d && !d->points.empty()) a.push_back(d->points[0]);
    for (const PointCloud<VFHSignature308>::Ptr& d : d2)
        if (d && !d->points.empty()) b.push_back(d->points[0]);
    std::vector<double> dist(a.size() * b.size());
    if (dist.empty()) return dist;  // (no library call)
    static_assert(sizeof(VFHSignature308) == 308 * sizeof(float), "descriptors lie 308 floats apart");
    check(pcc_match_vfh(detail::batchContext<PointXYZRGB>(ctx ? ctx->handle() : nullptr), a[0].histogram, a.size(), b[0].histogram, b.size(), PCC_MEM_HOST,
                        dist.data()));
    return dist;
}

}  // namespace pcc
