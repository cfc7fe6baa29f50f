// rgb_time.cpp -- dev helper of tools/exp_rgb.py: pcc::RegionGrowingRGB::extract on a PLY on its two paths -- the host logic
// over downloaded 100-neighbour rows, and setDeviceSegmentation(true) = one pcc_region_growing_rgb call -- on the same tree in
// this one process, alternating: 3 warm-ups, then R timed repetitions each (default 20).  Prints "time <points> <host ms>
// <device ms> <segments> <pairs> <sweeps> <clusters>" (medians of the host clock around extract(); the index build is part of
// both) after checking that the two paths return the same clusters.
// usage: rgb_time FILE.ply [R]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include "ply_io.hpp"
#include "pcc/region_growing_rgb.hpp"
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    pcc::PointCloud<pcc::PointXYZRGB>::Ptr c(new pcc::PointCloud<pcc::PointXYZRGB>);
    if (pcc::io::loadPLYFile(argv[1], *c) == -1) { std::printf("LOAD_FAILED\n"); return 1; }
    std::vector<int> idx;
    pcc::io::removeNaNFromPointCloud(*c, idx);
    const int reps = std::max(1, argc > 2 ? std::atoi(argv[2]) : 20);
    pcc::search::KdTree<pcc::PointXYZRGB>::Ptr tree(new pcc::search::KdTree<pcc::PointXYZRGB>);
    std::vector<double> ms[2];
    std::vector<pcc::PointIndices> out[2];
    uint64_t stats[8] = {0};
    for (int r = 0; r < reps + 3; ++r)
        for (int dev = 0; dev < 2; ++dev) {
            pcc::RegionGrowingRGB<pcc::PointXYZRGB> reg;  // color_growing_segmentation's settings
            reg.setInputCloud(c);
            reg.setSearchMethod(tree);
            reg.setDistanceThreshold(10);
            reg.setPointColorThreshold(6);
            reg.setRegionColorThreshold(5);
            reg.setMinClusterSize(200);
            reg.setDeviceSegmentation(dev == 1);
            const auto t0 = std::chrono::steady_clock::now();
            reg.extract(out[dev]);
            const double t = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (r >= 3) ms[dev].push_back(t);
            if (dev == 1 && tree->handle()) pcc_index_stats(tree->handle(), stats);
        }
    bool same = out[0].size() == out[1].size();
    for (size_t k = 0; same && k < out[0].size(); ++k) same = out[0][k].indices == out[1][k].indices;
    if (!same) { std::printf("PATHS_DIFFER\n"); return 1; }
    for (auto& v : ms) std::sort(v.begin(), v.end());
    std::printf("time %zu %.3f %.3f %llu %llu %llu %zu\n", c->size(), ms[0][ms[0].size() / 2], ms[1][ms[1].size() / 2],
                (unsigned long long)stats[0], (unsigned long long)stats[1], (unsigned long long)stats[7], out[1].size());
    return 0;
}
