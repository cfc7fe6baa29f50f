// cluster_desc_driver.cpp -- pcc::clusterDescriptors (include/pcc/descriptors.hpp: the reference's per-cluster descriptor loop,
// src/comparator.cpp:1224-1290, in one library call) on a file of clusters, for tests/test_cluster_desc_gpu.py: the C++ surface
// must return what Index.cluster_descriptors returns for the same clusters.
// usage: cluster_desc_driver IN OUT [SIFT_ABOVE]   (default 700)
//   IN:  int32 n_clusters, then per cluster int32 n + n x (x, y, z, colour word)
//   OUT: int32 n_clusters, then per cluster int32 m, int32 keypoints, 3 floats centroid, m x 32 floats, m x int32 point index
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "pcc/descriptors.hpp"

namespace {
struct Rec { float x, y, z; uint32_t bgra; };
typedef pcc::PointCloud<pcc::PointXYZRGB>::Ptr CloudPtr;
}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: cluster_desc_driver IN OUT [SIFT_ABOVE]\n"); return 2; }
    const size_t sift_above = argc > 3 ? (size_t)strtoull(argv[3], nullptr, 10) : pcc::SIFT_ABOVE;
    FILE* f = fopen(argv[1], "rb");
    int32_t nc = 0;
    if (!f || fread(&nc, 4, 1, f) != 1 || nc < 0) { fprintf(stderr, "cluster_desc_driver: cannot read %s\n", argv[1]); return 2; }
    std::vector<CloudPtr> clusters;
    for (int32_t c = 0; c < nc; ++c) {
        int32_t n = 0;
        if (fread(&n, 4, 1, f) != 1 || n < 0) { fprintf(stderr, "cluster_desc_driver: %s is short\n", argv[1]); return 2; }
        std::vector<Rec> rec((size_t)n);
        if (n && fread(rec.data(), sizeof(Rec), rec.size(), f) != rec.size()) { fprintf(stderr, "cluster_desc_driver: %s is short\n", argv[1]); return 2; }
        CloudPtr cloud(new pcc::PointCloud<pcc::PointXYZRGB>);
        for (const Rec& r : rec) {
            pcc::PointXYZRGB p;
            p.x = r.x; p.y = r.y; p.z = r.z; p.rgba = r.bgra;
            cloud->push_back(p);
        }
        clusters.push_back(cloud);
    }
    fclose(f);
    pcc::ClusterDescriptors res;
    try {
        res = pcc::clusterDescriptors(clusters, sift_above);
    } catch (const std::exception& e) {
        fprintf(stderr, "cluster_desc_driver: %s\n", e.what());
        return 1;
    }
    FILE* o = fopen(argv[2], "wb");
    bool ok = o != nullptr && fwrite(&nc, 4, 1, o) == 1;
    size_t descriptors = 0, keypoints = 0;
    for (size_t c = 0; ok && c < clusters.size(); ++c) {
        const int32_t m = (int32_t)res.descriptors[c]->size(), k = (int32_t)res.n_keypoints[c];
        const float cen[3] = {res.centroids[c].x, res.centroids[c].y, res.centroids[c].z};
        ok = fwrite(&m, 4, 1, o) == 1 && fwrite(&k, 4, 1, o) == 1 && fwrite(cen, 4, 3, o) == 3;
        for (int32_t i = 0; ok && i < m; ++i) ok = fwrite(res.descriptors[c]->points[i].histogram, 4, 32, o) == 32;
        for (int32_t i = 0; ok && i < m; ++i) {
            const int32_t idx = res.point_indices[c][i];
            ok = fwrite(&idx, 4, 1, o) == 1;
        }
        descriptors += (size_t)m;
        keypoints += (size_t)k;
    }
    if (!ok || fclose(o) != 0) { fprintf(stderr, "cluster_desc_driver: cannot write %s\n", argv[2]); return 2; }
    printf("cluster_desc_driver clusters=%zu keypoints=%zu descriptors=%zu\n", clusters.size(), keypoints, descriptors);
    return 0;
}
