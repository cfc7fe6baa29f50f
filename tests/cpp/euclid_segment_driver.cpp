// euclid_segment_driver.cpp -- pcc::euclideanClusterSegmentation against the objects it replaces (include/pcc/comparator_nn.hpp):
// the VoxelGrid + SACSegmentation / ExtractIndices loop + KdTree + EuclideanClusterExtraction sequence of the reference's -e path
// (src/segmentation.cpp:64-156), as examples/comparator_main.cpp drives it, and the one library call on the same small cloud.  The
// planes, the remaining cloud and every cluster cloud must be byte-equal.  argv[1], argv[2] (optional): the room for planes and
// clusters the mirror starts with (1 1: both repeats after an overflow).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "pcc/comparator_nn.hpp"

using namespace pcc;

// a 32-bit generator of the driver's own
static uint32_t g_state = 2463534242u;
static float rnd() {
    g_state ^= g_state << 13; g_state ^= g_state >> 17; g_state ^= g_state << 5;
    return (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

// a floor and a wall of side x side points and three boxes on a 0.03 lattice with a little jitter (one point per 0.025 voxel),
// colour, a box too small for a cluster and one non-finite point
static PointCloud<PointXYZRGB>::Ptr scene(int side) {
    PointCloud<PointXYZRGB>::Ptr c(new PointCloud<PointXYZRGB>);
    auto add = [&](float x, float y, float z) {
        PointXYZRGB p;
        p.x = x + 1.0f + (rnd() - 0.5f) * 0.004f; p.y = y + 1.0f + (rnd() - 0.5f) * 0.004f; p.z = z + 1.0f + (rnd() - 0.5f) * 0.004f;
        p.rgba = ((uint32_t)c->points.size() * 2654435761u) & 0xffffffu;
        c->points.push_back(p);
    };
    for (int i = 0; i < side; ++i)
        for (int j = 0; j < side; ++j) {
            add(0.03f * i, 0.03f * j, 0.f);
            add(-0.06f, 0.03f * i + 0.03f, 0.03f * j + 0.03f);
        }
    auto box = [&](int nx, int ny, int nz, float x, float y, float z) {
        for (int i = 0; i < nx; ++i)
            for (int j = 0; j < ny; ++j)
                for (int k = 0; k < nz; ++k) add(x + 0.03f * i, y + 0.03f * j, z + 0.03f * k);
    };
    box(6, 6, 6, 0.15f, 0.15f, 0.3f);
    box(6, 6, 6, 0.75f, 0.15f, 0.45f);
    box(7, 6, 6, 0.15f, 0.75f, 0.6f);
    box(5, 5, 3, 0.75f, 0.75f, 0.3f);
    c->points[5].z = std::nanf("");
    c->width = (std::uint32_t)c->points.size();
    c->height = 1;
    return c;
}

struct ClassResult {
    size_t n_filtered = 0;
    std::vector<std::uint32_t> sizes;
    std::vector<std::array<float, 4> > coefficients;
    bool ended = false;
    PointCloud<PointXYZRGB>::Ptr remaining;
    std::vector<PointCloud<PointXYZRGB>::Ptr> clusters;
};

static ClassResult class_path(const PointCloud<PointXYZRGB>::Ptr& cloud, float leaf, double stop) {
    ClassResult r;
    VoxelGrid<PointXYZRGB> vg;
    PointCloud<PointXYZRGB>::Ptr cur(new PointCloud<PointXYZRGB>);
    vg.setInputCloud(cloud);
    vg.setLeafSize(leaf, leaf, leaf);
    vg.filter(*cur);
    r.n_filtered = cur->points.size();
    SACSegmentation<PointXYZRGB> seg;
    seg.setOptimizeCoefficients(true);
    seg.setModelType(SACMODEL_PLANE);
    seg.setMethodType(SAC_RANSAC);
    seg.setMaxIterations(100);
    seg.setDistanceThreshold(0.02);
    const int nr_points = (int)cur->points.size();
    while (cur->points.size() > stop * nr_points) {
        std::shared_ptr<PointIndices> inliers(new PointIndices);
        ModelCoefficients mc;
        seg.setInputCloud(cur);
        seg.segment(*inliers, mc);
        if (inliers->indices.empty()) { r.ended = true; break; }
        r.sizes.push_back((std::uint32_t)inliers->indices.size());
        r.coefficients.push_back({mc.values[0], mc.values[1], mc.values[2], mc.values[3]});
        ExtractIndices<PointXYZRGB> extract;
        extract.setInputCloud(cur);
        extract.setIndices(inliers);
        extract.setNegative(true);
        PointCloud<PointXYZRGB>::Ptr rest(new PointCloud<PointXYZRGB>);
        extract.filter(*rest);
        cur = rest;
    }
    r.remaining = cur;
    search::KdTree<PointXYZRGB>::Ptr tree(new search::KdTree<PointXYZRGB>);
    tree->setInputCloud(cur);
    std::vector<PointIndices> found;
    EuclideanClusterExtraction<PointXYZRGB> ec;
    ec.setClusterTolerance(0.05);
    ec.setMinClusterSize(100);
    ec.setMaxClusterSize(250000);
    ec.setSearchMethod(tree);
    ec.setInputCloud(cur);
    ec.extract(found);
    for (const PointIndices& c : found) {
        PointCloud<PointXYZRGB>::Ptr one(new PointCloud<PointXYZRGB>);
        for (int j : c.indices) one->points.push_back(cur->points[j]);
        r.clusters.push_back(one);
    }
    return r;
}

static bool same_cloud(const PointCloud<PointXYZRGB>& a, const PointCloud<PointXYZRGB>& b) {
    return a.points.size() == b.points.size() &&
           (a.points.empty() || std::memcmp(a.points.data(), b.points.data(), a.points.size() * sizeof(PointXYZRGB)) == 0);
}

int main(int argc, char** argv) {
    const size_t first_planes = argc > 1 ? (size_t)std::atoi(argv[1]) : 64, first_clusters = argc > 2 ? (size_t)std::atoi(argv[2]) : 256;
    int failures = 0;
    struct Case { const char* name; int side; float leaf; double stop; size_t planes, clusters; };  // (clusters 0: whatever the objects find)
    // (1e-7: more voxels than the voxel grid takes -- PCL's "leaf size is too small", output = input -- the class path on both sides)
    for (const Case& k : {Case{"room 36", 36, 0.025f, 0.3, 2, 3}, Case{"room 30", 30, 0.025f, 0.3, 2, 3},
                          Case{"room 36, no plane", 36, 0.025f, 1.0, 0, 0}, Case{"room 30, leaf too small", 30, 1e-7f, 0.3, 2, 3}}) {
        PointCloud<PointXYZRGB>::Ptr cloud = scene(k.side);
        const ClassResult want = class_path(cloud, k.leaf, k.stop);
        for (int round = 0; round < 2; ++round) {  // (the second call reuses the thread's context and its work handle)
            RemovedPlanes planes;
            PointCloud<PointXYZRGB>::Ptr remaining;
            size_t n_filtered = 0;
            std::vector<PointCloud<PointXYZRGB>::Ptr> got = euclideanClusterSegmentation<PointXYZRGB>(
                cloud, k.leaf, k.stop, 100, 0.02, true, 0.05, 100, 250000, planes, &remaining, &n_filtered, first_planes, first_clusters);
            bool ok = got.size() == want.clusters.size() && (k.clusters == 0 || got.size() == k.clusters) && n_filtered == want.n_filtered &&
                      planes.sizes == want.sizes && planes.sizes.size() == k.planes && planes.ended_without_model == want.ended &&
                      planes.coefficients.size() == want.coefficients.size() && same_cloud(*remaining, *want.remaining);
            for (size_t p = 0; ok && p < want.coefficients.size(); ++p)
                ok = std::memcmp(planes.coefficients[p].data(), want.coefficients[p].data(), 4 * sizeof(float)) == 0;
            for (size_t c = 0; ok && c < got.size(); ++c) ok = same_cloud(*got[c], *want.clusters[c]) && got[c]->width == got[c]->points.size();
            std::printf("%s, call %d: %zu filtered points, %zu planes, %zu remain, %zu clusters: %s\n", k.name, round, n_filtered,
                        planes.sizes.size(), remaining->points.size(), got.size(), ok ? "equal" : "DIFFERENT");
            if (!ok) ++failures;
        }
    }
    // nothing in, nothing out
    {
        PointCloud<PointXYZRGB>::Ptr empty(new PointCloud<PointXYZRGB>), remaining;
        RemovedPlanes planes;
        const bool ok = euclideanClusterSegmentation<PointXYZRGB>(empty, 0.025f, 0.3, 100, 0.02, true, 0.05, 100, 250000, planes, &remaining).empty() &&
                        remaining && remaining->points.empty() && planes.sizes.empty();
        std::printf("empty cloud: %s\n", ok ? "empty" : "NOT EMPTY");
        if (!ok) ++failures;
    }
    if (failures) { std::printf("euclid segment driver: %d FAILURES\n", failures); return 1; }
    std::printf("euclid segment driver ok\n");
    return 0;
}
