// spatial_change.cpp -- the reference's spatial_change_detection (src/comparator.cpp:54-110) as a tool over
// pcc::spatialChangeDetection: its two-file signature, the resolution it hard-codes (32) as an argument, and the diff cloud it
// shows in a viewer written to a PLY instead (x, y, z, red, green, blue; binary).
//   spatial_change A.ply B.ply RES OUT.ply
// prints "Points of B in voxels A leaves empty: N".  tests/test_change_detection_gpu.py compares the file with the restatement.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include "ply_io.hpp"
#include "pcc/octree.hpp"

int main(int argc, char** argv) {
    if (argc != 5) {
        std::printf("usage: spatial_change A.ply B.ply RES OUT.ply\n");
        return 2;
    }
    pcc::PointCloud<pcc::PointXYZRGB>::Ptr cloudA(new pcc::PointCloud<pcc::PointXYZRGB>), cloudB(new pcc::PointCloud<pcc::PointXYZRGB>);
    if (pcc::io::loadPLYFile(argv[1], *cloudA) == -1) { std::printf("Was not able to open file \"%s\".\n", argv[1]); return 1; }
    if (pcc::io::loadPLYFile(argv[2], *cloudB) == -1) { std::printf("Was not able to open file \"%s\".\n", argv[2]); return 1; }
    pcc::PointCloud<pcc::PointXYZRGB>::Ptr cloudDiff;
    try {
        cloudDiff = pcc::spatialChangeDetection<pcc::PointXYZRGB>(cloudA, cloudB, std::atof(argv[3]));
    } catch (const pcc::Error& e) {
        std::printf("ERROR %d %s\n", e.status, e.what());
        return 1;
    }
    std::printf("Points of B in voxels A leaves empty: %zu\n", cloudDiff->size());
    if (pcc::io::savePLYFileBinary(argv[4], *cloudDiff) == -1) { std::printf("WRITE_FAILED\n"); return 1; }
    return 0;
}
