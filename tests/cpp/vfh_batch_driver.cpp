// vfh_batch_driver.cpp -- pcc::processVHFBatch and the matrix overload of pcc::matchVHF (include/pcc/vfh.hpp: processVHF for every
// cluster in one library call, every distance between two such results in another) on cloud files, for
// tests/test_vfh_batch_gpu.py: the batch must return what the loop of pcc::processVHF returns, cloud by cloud.
// usage: vfh_batch_driver OUT_PREFIX SPLIT IN...   (the files of tests/cpp/vfh_host.cpp: int32 n + n x (x, y, z, colour word) in;
//                                                  OUT_PREFIX.<c>: int32 m + m x 308 floats, m = 0 or 1;
//                                                  OUT_PREFIX.match: int32 n1, int32 n2, n1 x n2 doubles -- matchVHF of the
//                                                  descriptors of the first SPLIT clouds against those of the rest)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "pcc/vfh.hpp"

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: vfh_batch_driver OUT_PREFIX SPLIT IN...\n"); return 2; }
    struct Rec { float x, y, z; uint32_t bgra; };
    const size_t split = (size_t)strtoul(argv[2], nullptr, 10);
    std::vector<pcc::PointCloud<pcc::PointXYZRGB>::Ptr> clouds;
    for (int a = 3; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        int32_t n = 0;
        if (!f || fread(&n, 4, 1, f) != 1 || n < 0) { fprintf(stderr, "vfh_batch_driver: cannot read %s\n", argv[a]); return 2; }
        std::vector<Rec> rec((size_t)n);
        if (n && fread(rec.data(), sizeof(Rec), rec.size(), f) != rec.size()) { fprintf(stderr, "vfh_batch_driver: %s is short\n", argv[a]); return 2; }
        fclose(f);
        pcc::PointCloud<pcc::PointXYZRGB>::Ptr cloud(new pcc::PointCloud<pcc::PointXYZRGB>);
        for (const Rec& r : rec) {
            pcc::PointXYZRGB p;
            p.x = r.x; p.y = r.y; p.z = r.z; p.rgba = r.bgra;
            cloud->push_back(p);
        }
        clouds.push_back(cloud);
    }
    if (split > clouds.size()) { fprintf(stderr, "vfh_batch_driver: SPLIT beyond the clouds\n"); return 2; }
    std::vector<pcc::PointCloud<pcc::VFHSignature308>::Ptr> des;
    std::vector<double> dist;
    size_t differ = 0, rows = 0, n1 = 0, n2 = 0;
    try {
        des = pcc::processVHFBatch(clouds);
        for (size_t c = 0; c < clouds.size(); ++c) {
            const pcc::PointCloud<pcc::VFHSignature308>::Ptr one = pcc::processVHF(clouds[c]);
            bool same = one->size() == des[c]->size();
            for (size_t i = 0; same && i < one->size(); ++i)
                same = memcmp(one->points[i].histogram, des[c]->points[i].histogram, sizeof(one->points[i].histogram)) == 0;
            differ += same ? 0 : 1;
            rows += des[c]->size();
            (c < split ? n1 : n2) += des[c]->size();
        }
        const std::vector<pcc::PointCloud<pcc::VFHSignature308>::Ptr> d1(des.begin(), des.begin() + split), d2(des.begin() + split, des.end());
        dist = pcc::matchVHF(d1, d2);
        if (dist.size() != n1 * n2) { fprintf(stderr, "vfh_batch_driver: matchVHF returned %zu distances for %zu x %zu\n", dist.size(), n1, n2); return 1; }
    } catch (const std::exception& e) {
        fprintf(stderr, "vfh_batch_driver: %s\n", e.what());
        return 1;
    }
    for (size_t c = 0; c < clouds.size(); ++c) {
        const std::string name = std::string(argv[1]) + "." + std::to_string(c);
        const int32_t m = (int32_t)des[c]->size();
        FILE* f = fopen(name.c_str(), "wb");
        bool ok = f && fwrite(&m, 4, 1, f) == 1;
        for (int32_t i = 0; ok && i < m; ++i) ok = fwrite(des[c]->points[i].histogram, 4, 308, f) == 308;
        if (!ok || fclose(f) != 0) { fprintf(stderr, "vfh_batch_driver: cannot write %s\n", name.c_str()); return 2; }
    }
    {
        const std::string name = std::string(argv[1]) + ".match";
        const int32_t dims[2] = {(int32_t)n1, (int32_t)n2};
        FILE* f = fopen(name.c_str(), "wb");
        bool ok = f && fwrite(dims, 4, 2, f) == 2;
        if (ok && !dist.empty()) ok = fwrite(dist.data(), 8, dist.size(), f) == dist.size();
        if (!ok || fclose(f) != 0) { fprintf(stderr, "vfh_batch_driver: cannot write %s\n", name.c_str()); return 2; }
    }
    printf("vfh_batch_driver clouds=%zu descriptors=%zu differ_from_loop=%zu\n", clouds.size(), rows, differ);
    return differ ? 1 : 0;
}
