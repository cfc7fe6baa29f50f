// sift_driver.cpp -- pcc::processSift and pcc::processRIFTwithSIFT (include/pcc/sift.hpp, the reference's processSift
// src/comparator.cpp:435-469 and processRIFTwithSIFT :686-822) on a cloud file, for tests/test_sift_gpu.py: the C++ surface
// must return what Index.sift_keypoints, Index.first_within and Index.rift_descriptors return.
// usage: sift_driver IN OUT   (IN as for tests/cpp/sift_host.cpp: int32 n + n x (x, y, z, colour word);
//                              OUT: int32 m + m x (x, y, z, scale), then int32 n_des + n_des x 32 floats + n_des x int32
//                              indices into the snapped cloud)
#include <cstdint>
#include <cstdio>
#include <vector>
#include "pcc/sift.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: sift_driver IN OUT\n"); return 2; }
    struct Rec { float x, y, z; uint32_t bgra; };
    FILE* f = fopen(argv[1], "rb");
    int32_t n = 0;
    if (!f || fread(&n, 4, 1, f) != 1 || n < 0) { fprintf(stderr, "sift_driver: cannot read %s\n", argv[1]); return 2; }
    std::vector<Rec> rec((size_t)n);
    if (n && fread(rec.data(), sizeof(Rec), rec.size(), f) != rec.size()) { fprintf(stderr, "sift_driver: %s is short\n", argv[1]); return 2; }
    fclose(f);
    pcc::PointCloud<pcc::PointXYZRGB>::Ptr cloud(new pcc::PointCloud<pcc::PointXYZRGB>);
    for (const Rec& r : rec) {
        pcc::PointXYZRGB p;
        p.x = r.x; p.y = r.y; p.z = r.z; p.rgba = r.bgra;
        cloud->push_back(p);
    }
    pcc::PointCloud<pcc::PointWithScale>::Ptr kp;
    pcc::PointCloud<pcc::RIFT32>::Ptr des;
    std::vector<int> index;
    size_t n_kp = 0;
    try {
        kp = pcc::processSift(cloud);
        des = pcc::processRIFTwithSIFT(cloud, &index, &n_kp);
    } catch (const std::exception& e) {
        fprintf(stderr, "sift_driver: %s\n", e.what());
        return 1;
    }
    if (n_kp != kp->size()) { fprintf(stderr, "sift_driver: processRIFTwithSIFT saw %zu keypoints, processSift %zu\n", n_kp, kp->size()); return 1; }
    const int32_t m = (int32_t)kp->size(), n_des = (int32_t)des->size();
    f = fopen(argv[2], "wb");
    bool ok = f && fwrite(&m, 4, 1, f) == 1;
    for (int32_t i = 0; ok && i < m; ++i) {
        const float v[4] = {kp->points[i].x, kp->points[i].y, kp->points[i].z, kp->points[i].scale};
        ok = fwrite(v, 4, 4, f) == 4;
    }
    ok = ok && fwrite(&n_des, 4, 1, f) == 1;
    for (int32_t i = 0; ok && i < n_des; ++i) ok = fwrite(des->points[i].histogram, 4, 32, f) == 32;
    for (int32_t i = 0; ok && i < n_des; ++i) { const int32_t v = index[i]; ok = fwrite(&v, 4, 1, f) == 1; }
    if (!ok || fclose(f) != 0) { fprintf(stderr, "sift_driver: cannot write %s\n", argv[2]); return 2; }
    printf("sift_driver n=%d keypoints=%d descriptors=%d\n", n, m, n_des);
    return 0;
}
