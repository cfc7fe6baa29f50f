// rgb_segments_batch.cpp -- test helper: build/rgb_segments' output for SEVERAL PLY files, one after the other, from batch calls:
// the labels of every file from one pcc_region_growing_rgb_batch call with the four parameters (pcc::detail::rgbBatchCall), the
// "segments" line of every file from one pcc::color_growing_segmentation_batch call (the reference's defaults,
// src/segmentation.cpp:161-216).  tests/test_rgb_batch_gpu.py requires the output to be that of build/rgb_segments, file by file.
// usage: rgb_segments_batch A.ply [B.ply ...] [distance point_colour region_colour min_size]
#include <cstdio>
#include <cstdlib>
#include <string>
#include "ply_io.hpp"
#include "pcc/region_growing_rgb.hpp"
int main(int argc, char** argv) {
    typedef pcc::PointCloud<pcc::PointXYZRGB>::Ptr Ptr;
    std::vector<Ptr> clouds;
    std::vector<const char*> par;
    for (int a = 1; a < argc; ++a) {
        const std::string arg = argv[a];
        if (arg.size() > 4 && arg.substr(arg.size() - 4) == ".ply") {
            Ptr c(new pcc::PointCloud<pcc::PointXYZRGB>);
            if (pcc::io::loadPLYFile(arg, *c) == -1) { std::printf("LOAD_FAILED\n"); return 1; }
            std::vector<int> idx;
            pcc::io::removeNaNFromPointCloud(*c, idx);
            clouds.push_back(c);
        } else {
            par.push_back(argv[a]);
        }
    }
    if (clouds.empty()) return 2;
    std::vector<int32_t> labels, n_clusters;
    std::vector<size_t> offsets;
    std::vector<std::vector<Ptr> > segments;
    try {
        pcc::detail::rgbBatchCall<pcc::PointXYZRGB>(clouds, par.size() > 0 ? (float)std::atof(par[0]) : 10.f, par.size() > 1 ? (float)std::atof(par[1]) : 6.f,
                                                    par.size() > 2 ? (float)std::atof(par[2]) : 5.f, par.size() > 3 ? std::atoi(par[3]) : 200, nullptr,
                                                    labels, offsets, n_clusters);
        segments = pcc::color_growing_segmentation_batch<pcc::PointXYZRGB>(clouds);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "rgb_segments_batch: %s\n", e.what());
        return 1;
    }
    for (size_t c = 0; c < clouds.size(); ++c) {
        std::printf("%d %zu\n", (int)n_clusters[c], clouds[c]->size());
        for (size_t i = offsets[c]; i < offsets[c + 1]; ++i) std::printf("%d\n", (int)labels[i]);
        std::printf("segments %zu\n", segments[c].size());
    }
    return 0;
}
