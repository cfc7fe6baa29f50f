// plane_removal_driver.cpp -- pcc::removePlanes against the loop it replaces (include/pcc/comparator_nn.hpp): the
// SACSegmentation::segment + ExtractIndices loop of the reference's -e path (src/segmentation.cpp:79-117) and the one library
// call on the same small cloud.  The remaining clouds must be byte-equal, the planes equal.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "pcc/comparator_nn.hpp"

using namespace pcc;

// a 32-bit generator of the driver's own: three noisy planes, clutter, a few duplicates and one non-finite point, with colour
static uint32_t g_state = 2463534242u;
static float rnd() {
    g_state ^= g_state << 13; g_state ^= g_state >> 17; g_state ^= g_state << 5;
    return (float)(g_state >> 8) * (1.0f / 16777216.0f);
}

static PointCloud<PointXYZRGB>::Ptr scene() {
    PointCloud<PointXYZRGB>::Ptr c(new PointCloud<PointXYZRGB>);
    auto add = [&](float x, float y, float z) {
        PointXYZRGB p;
        p.x = x; p.y = y; p.z = z;
        p.rgba = (uint32_t)c->points.size() * 2654435761u;
        c->points.push_back(p);
    };
    for (int i = 0; i < 1500; ++i) {
        const int kind = i % 10;
        const float u = rnd() * 3.f, v = rnd() * 3.f, e = (rnd() - 0.5f) * 0.01f;
        if (kind < 4) add(u, v, e);
        else if (kind < 7) add(-0.5f + e, u, v);
        else if (kind < 9) add(u, -0.25f + e, v);
        else add(rnd() * 3.f - 0.5f, u - 0.5f, v - 0.5f);
    }
    for (int i = 0; i < 40; ++i) c->points.push_back(c->points[(size_t)(rnd() * 1500.f) % 1500]);  // duplicates
    c->points[17].y = std::nanf("");
    c->width = (std::uint32_t)c->points.size();
    c->height = 1;
    return c;
}

int main() {
    PointCloud<PointXYZRGB>::Ptr cloud = scene();
    int failures = 0;
    for (double stop : {0.3, 0.1, 1.0}) {
        // the loop as examples/comparator_main.cpp runs it
        SACSegmentation<PointXYZRGB> seg;
        seg.setOptimizeCoefficients(true);
        seg.setModelType(SACMODEL_PLANE);
        seg.setMethodType(SAC_RANSAC);
        seg.setMaxIterations(100);
        seg.setDistanceThreshold(0.02);
        PointCloud<PointXYZRGB>::Ptr cur(new PointCloud<PointXYZRGB>(*cloud));
        std::vector<std::uint32_t> sizes;
        std::vector<std::array<float, 4> > coefficients;
        bool ended = false;
        const int nr_points = (int)cur->points.size();
        while (cur->points.size() > stop * nr_points) {
            std::shared_ptr<PointIndices> inliers(new PointIndices);
            ModelCoefficients mc;
            seg.setInputCloud(cur);
            seg.segment(*inliers, mc);
            if (inliers->indices.empty()) { ended = true; break; }
            sizes.push_back((std::uint32_t)inliers->indices.size());
            coefficients.push_back({mc.values[0], mc.values[1], mc.values[2], mc.values[3]});
            ExtractIndices<PointXYZRGB> extract;
            extract.setInputCloud(cur);
            extract.setIndices(inliers);
            extract.setNegative(true);
            PointCloud<PointXYZRGB>::Ptr rest(new PointCloud<PointXYZRGB>);
            extract.filter(*rest);
            cur = rest;
        }
        RemovedPlanes planes;
        PointCloud<PointXYZRGB>::Ptr got = removePlanes<PointXYZRGB>(cloud, planes, stop, 100, 0.02, true);
        bool ok = got->points.size() == cur->points.size() && planes.sizes == sizes && planes.ended_without_model == ended &&
                  planes.coefficients.size() == coefficients.size();
        if (ok && !cur->points.empty())
            ok = std::memcmp(got->points.data(), cur->points.data(), cur->points.size() * sizeof(PointXYZRGB)) == 0;
        for (size_t p = 0; ok && p < coefficients.size(); ++p)
            ok = std::memcmp(planes.coefficients[p].data(), coefficients[p].data(), 4 * sizeof(float)) == 0;
        std::printf("stop %.1f: %zu planes, %zu of %zu points remain: %s\n", stop, sizes.size(), cur->points.size(), cloud->points.size(),
                    ok ? "equal" : "DIFFERENT");
        if (!ok) ++failures;
        if (stop == 0.3 && sizes.size() < 2) { std::printf("the scene lost its planes\n"); ++failures; }
    }
    // the capacity of 64 planes grown once: a threshold that leaves every plane a handful of points
    {
        RemovedPlanes planes;
        PointCloud<PointXYZRGB>::Ptr got = removePlanes<PointXYZRGB>(cloud, planes, 0.05, 100, 0.00005, true);
        size_t removed = 0;
        for (std::uint32_t s : planes.sizes) removed += s;
        const bool ok = planes.sizes.size() > 64 && removed + got->points.size() == cloud->points.size();
        std::printf("tight threshold: %zu planes, %zu remain: %s\n", planes.sizes.size(), got->points.size(), ok ? "grown" : "NOT GROWN");
        if (!ok) ++failures;
    }
    if (failures) { std::printf("plane removal driver: %d FAILURES\n", failures); return 1; }
    std::printf("plane removal driver ok\n");
    return 0;
}
