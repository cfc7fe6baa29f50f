// vfh.hpp -- pcc::processVHF and pcc::matchVHF: the reference's processVHF (src/comparator.cpp:482-516) and matchVHF (:471-480)
// re-hosted on libpcc_nn.  Same signatures and settings as the reference (normals at 0.03, setNormalizeBins(true),
// setNormalizeDistance(false)); the whole pipeline -- normals, the two centroids, one vote per point, the 308 bins -- is one
// pcc_vfh_descriptor call on a tree over the cloud, the distance one pcc_match_vfh call.  Like the reference's they print nothing.
#pragma once
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

}  // namespace pcc
