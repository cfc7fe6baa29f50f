// shot_driver.cpp -- pcc::processSHOT (include/pcc/shot.hpp, the reference's processSHOT src/comparator.cpp:941-986)
// on a cloud file, for tests/test_shot_gpu.py: the C++ mirror must return what Index.shot_descriptors returns.
// usage: shot_driver IN OUT   (the files of tests/cpp/shot_host.cpp: int32 n + n x (x, y, z, colour word) in,
//                              int32 m + m x 352 floats + m x 9 floats + m x int32 point indices out; the index of the
//                              fallback descriptor, which belongs to no point, is -1)
#include <cstdint>
#include <cstdio>
#include <vector>
#include "pcc/shot.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: shot_driver IN OUT\n"); return 2; }
    struct Rec { float x, y, z; uint32_t bgra; };
    FILE* f = fopen(argv[1], "rb");
    int32_t n = 0;
    if (!f || fread(&n, 4, 1, f) != 1 || n < 0) { fprintf(stderr, "shot_driver: cannot read %s\n", argv[1]); return 2; }
    std::vector<Rec> rec((size_t)n);
    if (n && fread(rec.data(), sizeof(Rec), rec.size(), f) != rec.size()) { fprintf(stderr, "shot_driver: %s is short\n", argv[1]); return 2; }
    fclose(f);
    pcc::PointCloud<pcc::PointXYZRGB>::Ptr cloud(new pcc::PointCloud<pcc::PointXYZRGB>);
    for (const Rec& r : rec) {
        pcc::PointXYZRGB p;
        p.x = r.x; p.y = r.y; p.z = r.z; p.rgba = r.bgra;
        cloud->push_back(p);
    }
    std::vector<int> index;
    pcc::PointCloud<pcc::SHOT352>::Ptr des;
    try {
        des = pcc::processSHOT(cloud, &index);
    } catch (const std::exception& e) {
        fprintf(stderr, "shot_driver: %s\n", e.what());
        return 1;
    }
    const int32_t n_out = (int32_t)des->size();
    f = fopen(argv[2], "wb");
    bool ok = f && fwrite(&n_out, 4, 1, f) == 1;
    for (int32_t i = 0; ok && i < n_out; ++i) ok = fwrite(des->points[i].descriptor, 4, 352, f) == 352;
    for (int32_t i = 0; ok && i < n_out; ++i) ok = fwrite(des->points[i].rf, 4, 9, f) == 9;
    for (int32_t i = 0; ok && i < n_out; ++i) { const int32_t v = (size_t)i < index.size() ? index[i] : -1; ok = fwrite(&v, 4, 1, f) == 1; }
    if (!ok || fclose(f) != 0) { fprintf(stderr, "shot_driver: cannot write %s\n", argv[2]); return 2; }
    printf("shot_driver n=%d kept=%d\n", n, n_out);
    return 0;
}
