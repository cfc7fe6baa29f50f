// vfh_driver.cpp -- pcc::processVHF and pcc::matchVHF (include/pcc/vfh.hpp, the reference's processVHF src/comparator.cpp:482-516
// and matchVHF :471-480) on cloud files, for tests/test_vfh_gpu.py: the C++ mirror must return what Index.vfh_descriptor and
// capi.match_vfh return.
// usage: vfh_driver IN OUT               (the files of tests/cpp/vfh_host.cpp: int32 n + n x (x, y, z, colour word) in,
//                                         int32 m + m x 308 floats out)
//        vfh_driver --match IN1 IN2 OUT  OUT = one double: matchVHF(processVHF(IN1), processVHF(IN2))
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "pcc/vfh.hpp"

static pcc::PointCloud<pcc::PointXYZRGB>::Ptr read_cloud(const char* path) {
    struct Rec { float x, y, z; uint32_t bgra; };
    FILE* f = fopen(path, "rb");
    int32_t n = 0;
    if (!f || fread(&n, 4, 1, f) != 1 || n < 0) { fprintf(stderr, "vfh_driver: cannot read %s\n", path); if (f) fclose(f); return nullptr; }
    std::vector<Rec> rec((size_t)n);
    const bool ok = !n || fread(rec.data(), sizeof(Rec), rec.size(), f) == rec.size();
    fclose(f);
    if (!ok) { fprintf(stderr, "vfh_driver: %s is short\n", path); return nullptr; }
    pcc::PointCloud<pcc::PointXYZRGB>::Ptr cloud(new pcc::PointCloud<pcc::PointXYZRGB>);
    for (const Rec& r : rec) {
        pcc::PointXYZRGB p;
        p.x = r.x; p.y = r.y; p.z = r.z; p.rgba = r.bgra;
        cloud->push_back(p);
    }
    return cloud;
}

int main(int argc, char** argv) {
    const bool match = argc == 5 && std::string(argv[1]) == "--match";
    if (!match && argc != 3) { fprintf(stderr, "usage: vfh_driver IN OUT\n       vfh_driver --match IN1 IN2 OUT\n"); return 2; }
    try {
        if (match) {
            pcc::PointCloud<pcc::PointXYZRGB>::Ptr c1 = read_cloud(argv[2]), c2 = read_cloud(argv[3]);
            if (!c1 || !c2) return 2;
            const double dis = pcc::matchVHF(pcc::processVHF(c1), pcc::processVHF(c2));
            FILE* f = fopen(argv[4], "wb");
            if (!f || fwrite(&dis, 8, 1, f) != 1 || fclose(f) != 0) { fprintf(stderr, "vfh_driver: cannot write %s\n", argv[4]); return 2; }
            printf("vfh_driver match %.17g\n", dis);
            return 0;
        }
        pcc::PointCloud<pcc::PointXYZRGB>::Ptr cloud = read_cloud(argv[1]);
        if (!cloud) return 2;
        pcc::PointCloud<pcc::VFHSignature308>::Ptr des = pcc::processVHF(cloud);
        const int32_t m = (int32_t)des->size();
        FILE* f = fopen(argv[2], "wb");
        bool ok = f && fwrite(&m, 4, 1, f) == 1;
        for (int32_t i = 0; ok && i < m; ++i) ok = fwrite(des->points[i].histogram, 4, 308, f) == 308;
        if (!ok || fclose(f) != 0) { fprintf(stderr, "vfh_driver: cannot write %s\n", argv[2]); return 2; }
        printf("vfh_driver n=%zu out=%d\n", cloud->size(), m);
    } catch (const std::exception& e) {
        fprintf(stderr, "vfh_driver: %s\n", e.what());
        return 1;
    }
    return 0;
}
