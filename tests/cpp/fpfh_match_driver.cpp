// fpfh_match_driver.cpp -- pcc::processFPFH on two cloud files, then pcc::matchFPFH on their descriptors (include/pcc/fpfh.hpp; the
// reference's processFPFH and matchFPFH, src/comparator.cpp:824-910), for tests/test_match_fpfh_gpu.py: the C++ mirror must return
// the row Index.match_fpfh_batch returns.
// usage: fpfh_match_driver IN1 IN2 OUT   (IN: the files of tests/cpp/fpfh_host.cpp, int32 n + n x (x, y, z, colour word);
//                                         OUT: int32 m + m x int32, the correspondence vector with its leading 0)
#include <cstdint>
#include <cstdio>
#include <vector>
#include "pcc/fpfh.hpp"

static bool read_cloud(const char* path, pcc::PointCloud<pcc::PointXYZRGB>::Ptr* cloud) {
    struct Rec { float x, y, z; uint32_t bgra; };
    FILE* f = fopen(path, "rb");
    int32_t n = 0;
    if (!f || fread(&n, 4, 1, f) != 1 || n < 0) { fprintf(stderr, "fpfh_match_driver: cannot read %s\n", path); return false; }
    std::vector<Rec> rec((size_t)n);
    if (n && fread(rec.data(), sizeof(Rec), rec.size(), f) != rec.size()) { fprintf(stderr, "fpfh_match_driver: %s is short\n", path); return false; }
    fclose(f);
    cloud->reset(new pcc::PointCloud<pcc::PointXYZRGB>);
    for (const Rec& r : rec) {
        pcc::PointXYZRGB p;
        p.x = r.x; p.y = r.y; p.z = r.z; p.rgba = r.bgra;
        (*cloud)->push_back(p);
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 4) { fprintf(stderr, "usage: fpfh_match_driver IN1 IN2 OUT\n"); return 2; }
    pcc::PointCloud<pcc::PointXYZRGB>::Ptr cloud1, cloud2;
    if (!read_cloud(argv[1], &cloud1) || !read_cloud(argv[2], &cloud2)) return 2;
    std::vector<int> correspondence;
    size_t m1 = 0, m2 = 0;
    try {
        pcc::PointCloud<pcc::FPFHSignature33>::Ptr des1 = pcc::processFPFH(cloud1), des2 = pcc::processFPFH(cloud2);
        m1 = des1->size();
        m2 = des2->size();
        correspondence = pcc::matchFPFH(des1, des2);
    } catch (const std::exception& e) {
        fprintf(stderr, "fpfh_match_driver: %s\n", e.what());
        return 1;
    }
    const int32_t m = (int32_t)correspondence.size();
    FILE* f = fopen(argv[3], "wb");
    bool ok = f && fwrite(&m, 4, 1, f) == 1;
    for (int32_t i = 0; ok && i < m; ++i) { const int32_t v = correspondence[i]; ok = fwrite(&v, 4, 1, f) == 1; }
    if (!ok || fclose(f) != 0) { fprintf(stderr, "fpfh_match_driver: cannot write %s\n", argv[3]); return 2; }
    printf("fpfh_match_driver des1=%zu des2=%zu kept=%d\n", m1, m2, m - 1);
    return 0;
}
