// fpfh_batch_driver.cpp -- pcc::processFPFHBatch (include/pcc/fpfh.hpp: processFPFH for every cluster in one library call) on
// cloud files, for tests/test_fpfh_batch_gpu.py: the batch must return what the loop of pcc::processFPFH returns, cloud by cloud.
// usage: fpfh_batch_driver OUT_PREFIX IN...   (the files of tests/cpp/fpfh_host.cpp: int32 n + n x (x, y, z, colour word) in;
//                                              OUT_PREFIX.<c>: int32 m + m x 33 floats + m x int32 point indices)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "pcc/fpfh.hpp"

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: fpfh_batch_driver OUT_PREFIX IN...\n"); return 2; }
    struct Rec { float x, y, z; uint32_t bgra; };
    std::vector<pcc::PointCloud<pcc::PointXYZRGB>::Ptr> clouds;
    for (int a = 2; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        int32_t n = 0;
        if (!f || fread(&n, 4, 1, f) != 1 || n < 0) { fprintf(stderr, "fpfh_batch_driver: cannot read %s\n", argv[a]); return 2; }
        std::vector<Rec> rec((size_t)n);
        if (n && fread(rec.data(), sizeof(Rec), rec.size(), f) != rec.size()) { fprintf(stderr, "fpfh_batch_driver: %s is short\n", argv[a]); return 2; }
        fclose(f);
        pcc::PointCloud<pcc::PointXYZRGB>::Ptr cloud(new pcc::PointCloud<pcc::PointXYZRGB>);
        for (const Rec& r : rec) {
            pcc::PointXYZRGB p;
            p.x = r.x; p.y = r.y; p.z = r.z; p.rgba = r.bgra;
            cloud->push_back(p);
        }
        clouds.push_back(cloud);
    }
    std::vector<std::vector<int>> index;
    std::vector<pcc::PointCloud<pcc::FPFHSignature33>::Ptr> des;
    size_t differ = 0, kept = 0;
    try {
        des = pcc::processFPFHBatch(clouds, nullptr, &index);
        for (size_t c = 0; c < clouds.size(); ++c) {
            std::vector<int> one_index;
            const pcc::PointCloud<pcc::FPFHSignature33>::Ptr one = pcc::processFPFH(clouds[c], &one_index);
            bool same = one->size() == des[c]->size() && one_index == index[c];
            for (size_t i = 0; same && i < one->size(); ++i)
                same = memcmp(one->points[i].histogram, des[c]->points[i].histogram, sizeof(one->points[i].histogram)) == 0;
            differ += same ? 0 : 1;
            kept += des[c]->size();
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "fpfh_batch_driver: %s\n", e.what());
        return 1;
    }
    for (size_t c = 0; c < clouds.size(); ++c) {
        const std::string name = std::string(argv[1]) + "." + std::to_string(c);
        const int32_t n_out = (int32_t)des[c]->size();
        FILE* f = fopen(name.c_str(), "wb");
        bool ok = f && fwrite(&n_out, 4, 1, f) == 1;
        for (int32_t i = 0; ok && i < n_out; ++i) ok = fwrite(des[c]->points[i].histogram, 4, 33, f) == 33;
        for (int32_t i = 0; ok && i < n_out; ++i) { const int32_t v = index[c][i]; ok = fwrite(&v, 4, 1, f) == 1; }
        if (!ok || fclose(f) != 0) { fprintf(stderr, "fpfh_batch_driver: cannot write %s\n", name.c_str()); return 2; }
    }
    printf("fpfh_batch_driver clouds=%zu kept=%zu differ_from_loop=%zu\n", clouds.size(), kept, differ);
    return differ ? 1 : 0;
}
