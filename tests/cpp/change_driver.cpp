// change_driver.cpp -- the reference's own call sequence (spatial_change_detection, src/comparator.cpp:74-92) against
// pcc::octree::OctreePointCloudChangeDetector (include/pcc/octree.hpp), and pcc::spatialChangeDetection on the same clouds.
//   change_driver A.bin B.bin RESOLUTION [MIN_POINTS_PER_LEAF]
// A.bin, B.bin: pcl::PointXYZRGB records (32 bytes each).  Prints "indices" and the result of the class, then whether the free
// function gave the same indices and the records they name; tests/test_change_detection_gpu.py compares with the Python call.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "pcc/octree.hpp"

static pcc::PointCloud<pcc::PointXYZRGB>::Ptr load(const char* path) {
    pcc::PointCloud<pcc::PointXYZRGB>::Ptr c(new pcc::PointCloud<pcc::PointXYZRGB>);
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return nullptr;
    pcc::PointXYZRGB p;
    while (std::fread(&p, sizeof(p), 1, f) == 1) c->points.push_back(p);
    std::fclose(f);
    c->width = (std::uint32_t)c->points.size();
    return c;
}

int main(int argc, char** argv) {
    if (argc < 4) { std::printf("usage: change_driver A.bin B.bin RESOLUTION [MIN_POINTS_PER_LEAF]\n"); return 2; }
    pcc::PointCloud<pcc::PointXYZRGB>::Ptr cloudA = load(argv[1]), cloudB = load(argv[2]);
    if (!cloudA || !cloudB) { std::printf("LOAD_FAILED\n"); return 1; }
    const float resolution = (float)std::atof(argv[3]);
    const int min_points = argc > 4 ? std::atoi(argv[4]) : 0;
    try {
        // Instantiate octree-based point cloud change detection class
        pcc::octree::OctreePointCloudChangeDetector<pcc::PointXYZRGB> octree(resolution);
        // Add points from cloudA to octree
        octree.setInputCloud(cloudA);
        octree.addPointsFromInputCloud();
        // Switch octree buffers
        octree.switchBuffers();
        // Add points from cloudB to octree
        octree.setInputCloud(cloudB);
        octree.addPointsFromInputCloud();
        std::vector<int> newPointIdxVector;
        // Get vector of point indices from octree voxels which did not exist in previous buffer
        if (min_points) octree.getPointIndicesFromNewVoxels(newPointIdxVector, min_points);
        else octree.getPointIndicesFromNewVoxels(newPointIdxVector);
        std::printf("indices");
        for (int i : newPointIdxVector) std::printf(" %d", i);
        std::printf("\n");

        std::vector<int> idx;
        pcc::PointCloud<pcc::PointXYZRGB>::Ptr diff = pcc::spatialChangeDetection<pcc::PointXYZRGB>(cloudA, cloudB, resolution, &idx, min_points);
        bool same = idx == newPointIdxVector && diff->size() == idx.size() && diff->width == idx.size();
        for (size_t j = 0; same && j < idx.size(); ++j) same = std::memcmp(&diff->points[j], &cloudB->points[idx[j]], sizeof(pcc::PointXYZRGB)) == 0;
        std::printf("free function: %s\n", same ? "same" : "DIFFERENT");
        // before any switchBuffers there is no previous buffer: every finite point is in a new voxel
        pcc::octree::OctreePointCloudChangeDetector<pcc::PointXYZRGB> fresh(resolution);
        fresh.setInputCloud(cloudB);
        fresh.addPointsFromInputCloud();
        std::vector<int> all;
        std::printf("no previous buffer: %zu\n", fresh.getPointIndicesFromNewVoxels(all));
        return same ? 0 : 1;
    } catch (const pcc::Error& e) {
        std::printf("ERROR %d %s\n", e.status, e.what());
        return 1;
    }
}
