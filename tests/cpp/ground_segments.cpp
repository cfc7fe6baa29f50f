// ground_segments.cpp -- the reference's ground_segmentation (src/segmentation.cpp:330-387) as a tool over pcc::groundSegmentation:
// a PLY in, <prefix>_ground.ply and <prefix>_object.ply out (x, y, z; binary), as the reference function writes
// samp11-utm_ground.ply and samp11-utm_object.ply.  tests/test_ground_cli_gpu.py compares the files with the Python call.
//   ground_segments in.ply prefix [leaf max_window slope initial_distance max_distance cell_size base exponential]
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include "ply_io.hpp"
#include "pcc/ground.hpp"

static int save_xyz(const std::string& path, const pcc::PointCloud<pcc::PointXYZ>& cloud) {
    std::ofstream f(path.c_str(), std::ios::binary);
    if (!f) return -1;
    f << "ply\nformat binary_little_endian 1.0\nelement vertex " << cloud.size() << "\nproperty float x\nproperty float y\nproperty float z\nend_header\n";
    for (const pcc::PointXYZ& p : cloud.points) f.write(reinterpret_cast<const char*>(&p.x), 12);
    return f ? 0 : -1;
}

int main(int argc, char** argv) {
    if (argc < 3) {
        std::printf("usage: ground_segments in.ply prefix [leaf max_window slope initial_distance max_distance cell_size base exponential]\n");
        return 2;
    }
    pcc::PointCloud<pcc::PointXYZRGB> in;
    if (pcc::io::loadPLYFile(argv[1], in) == -1) { std::printf("LOAD_FAILED\n"); return 1; }
    pcc::PointCloud<pcc::PointXYZ>::Ptr cloud(new pcc::PointCloud<pcc::PointXYZ>);
    cloud->points.resize(in.size());
    for (size_t i = 0; i < in.size(); ++i) { cloud->points[i].x = in[i].x; cloud->points[i].y = in[i].y; cloud->points[i].z = in[i].z; }
    cloud->width = (std::uint32_t)in.size();
    auto num = [&](int i, double dflt) { return argc > i ? std::atof(argv[i]) : dflt; };
    const std::string prefix = argv[2];
    pcc::PointCloud<pcc::PointXYZ> ground, object, filtered;
    try {
        pcc::groundSegmentation<pcc::PointXYZ>(cloud, ground, object, (float)num(3, 0.01), (int)num(4, 20), (float)num(5, 1.0), (float)num(6, 0.5),
                                               (float)num(7, 3.0), (float)num(8, 1.0), (float)num(9, 2.0), num(10, 1) != 0, &filtered);
        // and the filter's class over the filtered cloud gives the same ground
        pcc::ProgressiveMorphologicalFilter<pcc::PointXYZ> pmf;
        pmf.setInputCloud(std::make_shared<const pcc::PointCloud<pcc::PointXYZ>>(filtered));
        pmf.setMaxWindowSize((int)num(4, 20));
        pmf.setSlope((float)num(5, 1.0));
        pmf.setInitialDistance((float)num(6, 0.5));
        pmf.setMaxDistance((float)num(7, 3.0));
        pmf.setCellSize((float)num(8, 1.0));
        pmf.setBase((float)num(9, 2.0));
        pmf.setExponential(num(10, 1) != 0);
        std::vector<int> idx;
        pmf.extract(idx);
        std::printf("class_ground %zu\n", idx.size());
    } catch (const pcc::Error& e) {
        std::printf("ERROR %d %s\n", e.status, e.what());
        return 1;
    }
    std::printf("Ground cloud after filtering: %zu\nObject cloud after filtering: %zu\nfiltered %zu\n", ground.size(), object.size(), filtered.size());
    if (save_xyz(prefix + "_ground.ply", ground) || save_xyz(prefix + "_object.ply", object)) { std::printf("WRITE_FAILED\n"); return 1; }
    return 0;
}
