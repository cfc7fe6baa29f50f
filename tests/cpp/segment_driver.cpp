// segment_driver.cpp -- pcc::regionGrowingSegmentation against the objects it replaces (include/pcc/comparator_nn.hpp): the
// VoxelGrid + KdTree + NormalEstimation + RegionGrowing sequence of the reference's default path (src/segmentation.cpp:218-327),
// as examples/comparator_main.cpp drives it, and the one library call on the same small clouds.  The filtered clouds and every
// cluster cloud must be byte-equal.
#include <cmath>
#include <cstdio>
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

// three plates 0.28 apart on a 0.03 lattice with a little jitter (one point per 0.025 voxel), colour, a few stray points that
// join no cluster and one non-finite point
static PointCloud<PointXYZRGB>::Ptr scene(int side) {
    PointCloud<PointXYZRGB>::Ptr c(new PointCloud<PointXYZRGB>);
    auto add = [&](float x, float y, float z) {
        PointXYZRGB p;
        p.x = x + 1.0f; p.y = y + 1.0f; p.z = z + 1.0f;
        p.rgba = ((uint32_t)c->points.size() * 2654435761u) & 0xffffffu;
        c->points.push_back(p);
    };
    for (int i = 0; i < side; ++i)
        for (int j = 0; j < side; ++j) {
            const float u = 0.03f * i + (rnd() - 0.5f) * 0.004f, v = 0.03f * j + (rnd() - 0.5f) * 0.004f, e = (rnd() - 0.5f) * 0.002f;
            add(u, v, e);
            add(u, 1.0f + e, v + 0.2f);
            add(1.0f + e, u, v + 0.2f);
        }
    for (int i = 0; i < 20; ++i) add(2.0f + 0.03f * i, 2.0f, 2.0f);
    c->points[5].z = std::nanf("");
    c->width = (std::uint32_t)c->points.size();
    c->height = 1;
    return c;
}

static std::vector<PointCloud<PointXYZRGB>::Ptr> class_path(const PointCloud<PointXYZRGB>::Ptr& cloud, float leaf,
                                                            PointCloud<PointXYZRGB>::Ptr& cloud_filtered) {
    VoxelGrid<PointXYZRGB> vg;
    cloud_filtered.reset(new PointCloud<PointXYZRGB>);
    vg.setInputCloud(cloud);
    vg.setLeafSize(leaf, leaf, leaf);
    vg.filter(*cloud_filtered);
    search::KdTree<PointXYZRGB>::Ptr tree(new search::KdTree<PointXYZRGB>);
    tree->setOption(PCC_OPT_KNN_CACHE_K, 100);
    PointCloud<Normal>::Ptr normals(new PointCloud<Normal>);
    NormalEstimation<PointXYZRGB, Normal> ne;
    ne.setSearchMethod(tree);
    ne.setInputCloud(cloud_filtered);
    ne.setKSearch(50);
    ne.compute(*normals);
    RegionGrowing<PointXYZRGB, Normal> reg;
    reg.setMinClusterSize(50);
    reg.setMaxClusterSize(1000000);
    reg.setSearchMethod(tree);
    reg.setNumberOfNeighbours(100);
    reg.setInputCloud(cloud_filtered);
    reg.setInputNormals(normals);
    reg.setSmoothnessThreshold(3.0 / 180.0 * M_PI);
    reg.setCurvatureThreshold(1);
    std::vector<PointIndices> found;
    reg.extract(found);
    std::vector<PointCloud<PointXYZRGB>::Ptr> clusters;
    for (const PointIndices& c : found) {
        PointCloud<PointXYZRGB>::Ptr one(new PointCloud<PointXYZRGB>);
        for (int j : c.indices) one->points.push_back(cloud_filtered->points[j]);
        clusters.push_back(one);
    }
    return clusters;
}

static bool same_cloud(const PointCloud<PointXYZRGB>& a, const PointCloud<PointXYZRGB>& b) {
    return a.points.size() == b.points.size() &&
           (a.points.empty() || std::memcmp(a.points.data(), b.points.data(), a.points.size() * sizeof(PointXYZRGB)) == 0);
}

int main() {
    int failures = 0;
    struct Case { const char* name; int side; float leaf; size_t clusters; };
    // (1e-7: more voxels than the voxel grid takes -- PCL's "leaf size is too small", output = input -- the class path on both sides)
    for (const Case& k : {Case{"plates 20", 20, 0.025f, 3}, Case{"plates 27", 27, 0.025f, 3}, Case{"plates 20, leaf too small", 20, 1e-7f, 3}}) {
        PointCloud<PointXYZRGB>::Ptr cloud = scene(k.side);
        PointCloud<PointXYZRGB>::Ptr want_filtered, got_filtered;
        std::vector<PointCloud<PointXYZRGB>::Ptr> want = class_path(cloud, k.leaf, want_filtered);
        for (int round = 0; round < 2; ++round) {  // (the second call reuses the thread's context and its work handle)
            std::vector<PointCloud<PointXYZRGB>::Ptr> got = regionGrowingSegmentation<PointXYZRGB>(
                cloud, k.leaf, 50, 100, (float)(3.0 / 180.0 * M_PI), 1.0f, 50, 1000000, &got_filtered);
            bool ok = got.size() == want.size() && got.size() == k.clusters && same_cloud(*got_filtered, *want_filtered);
            for (size_t c = 0; ok && c < got.size(); ++c) ok = same_cloud(*got[c], *want[c]) && got[c]->width == got[c]->points.size();
            std::printf("%s, call %d: %zu filtered points, %zu clusters: %s\n", k.name, round, got_filtered->points.size(), got.size(),
                        ok ? "equal" : "DIFFERENT");
            if (!ok) ++failures;
        }
    }
    // nothing in, nothing out
    {
        PointCloud<PointXYZRGB>::Ptr empty(new PointCloud<PointXYZRGB>), filtered;
        const bool ok = regionGrowingSegmentation<PointXYZRGB>(empty, 0.025f, 50, 100, 0.05f, 1.0f, 50, 1000000, &filtered).empty() && filtered &&
                        filtered->points.empty();
        std::printf("empty cloud: %s\n", ok ? "empty" : "NOT EMPTY");
        if (!ok) ++failures;
    }
    // neighbour counts the library refuses are refused as such, not taken for a leaf that is too small
    {
        PointCloud<PointXYZRGB>::Ptr cloud = scene(20);
        int status = 0;
        try {
            regionGrowingSegmentation<PointXYZRGB>(cloud, 0.025f, 50, 0);
        } catch (const Error& e) {
            status = e.status;
        }
        std::printf("k = 0: %s\n", status == PCC_ERR_UNSUPPORTED ? "refused" : "NOT REFUSED");
        if (status != PCC_ERR_UNSUPPORTED) ++failures;
    }
    if (failures) { std::printf("segment driver: %d FAILURES\n", failures); return 1; }
    std::printf("segment driver ok\n");
    return 0;
}
