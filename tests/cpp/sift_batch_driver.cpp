// sift_batch_driver.cpp -- pcc::processSiftBatch and pcc::siftSnappedCloudBatch (include/pcc/sift.hpp: the front of the
// reference's processRIFTwithSIFT, src/comparator.cpp:686-822, for every cluster in one library call) on cloud files, for
// tests/test_sift_batch_gpu.py: the batch must return what the loop of pcc::processSift / pcc::siftSnappedCloud returns, cloud
// by cloud.  Both results are written; the test compares the bytes.
// usage: sift_batch_driver OUT_PREFIX IN...   (IN: int32 n + n x (x, y, z, colour word), the files of tests/cpp/sift_host.cpp)
//   OUT_PREFIX.batch / OUT_PREFIX.loop: per cloud int32 m, m x (x, y, z, scale), int32 k, k x (x, y, z, colour word) snapped points
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "pcc/sift.hpp"

namespace {

struct Rec { float x, y, z; uint32_t bgra; };
typedef pcc::PointCloud<pcc::PointXYZRGB>::Ptr CloudPtr;
typedef pcc::PointCloud<pcc::PointWithScale>::Ptr KeypointsPtr;

bool write_result(const std::string& name, const std::vector<KeypointsPtr>& kp, const std::vector<CloudPtr>& snapped) {
    FILE* f = fopen(name.c_str(), "wb");
    bool ok = f != nullptr;
    for (size_t c = 0; ok && c < kp.size(); ++c) {
        const int32_t m = (int32_t)kp[c]->size(), k = (int32_t)snapped[c]->size();
        ok = fwrite(&m, 4, 1, f) == 1;
        for (int32_t i = 0; ok && i < m; ++i) {
            const pcc::PointWithScale& p = kp[c]->points[i];
            const float v[4] = {p.x, p.y, p.z, p.scale};
            ok = fwrite(v, 4, 4, f) == 4;
        }
        ok = ok && fwrite(&k, 4, 1, f) == 1;
        for (int32_t i = 0; ok && i < k; ++i) {
            const pcc::PointXYZRGB& p = snapped[c]->points[i];
            const Rec r = {p.x, p.y, p.z, p.rgba};
            ok = fwrite(&r, sizeof(Rec), 1, f) == 1;
        }
    }
    return ok && fclose(f) == 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: sift_batch_driver OUT_PREFIX IN...\n"); return 2; }
    std::vector<CloudPtr> clouds;
    for (int a = 2; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        int32_t n = 0;
        if (!f || fread(&n, 4, 1, f) != 1 || n < 0) { fprintf(stderr, "sift_batch_driver: cannot read %s\n", argv[a]); return 2; }
        std::vector<Rec> rec((size_t)n);
        if (n && fread(rec.data(), sizeof(Rec), rec.size(), f) != rec.size()) { fprintf(stderr, "sift_batch_driver: %s is short\n", argv[a]); return 2; }
        fclose(f);
        CloudPtr cloud(new pcc::PointCloud<pcc::PointXYZRGB>);
        for (const Rec& r : rec) {
            pcc::PointXYZRGB p;
            p.x = r.x; p.y = r.y; p.z = r.z; p.rgba = r.bgra;
            cloud->push_back(p);
        }
        clouds.push_back(cloud);
    }
    std::vector<KeypointsPtr> kp_batch, kp_loop;
    std::vector<CloudPtr> snap_batch, snap_loop;
    std::vector<size_t> found;
    size_t keypoints = 0, snapped = 0;
    try {
        kp_batch = pcc::processSiftBatch(clouds);
        snap_batch = pcc::siftSnappedCloudBatch(clouds, &found);
        for (size_t c = 0; c < clouds.size(); ++c) {
            kp_loop.push_back(pcc::processSift(clouds[c]));
            size_t one = 0;
            snap_loop.push_back(pcc::siftSnappedCloud(clouds[c], &one));
            if (one != found[c] || one != kp_batch[c]->size()) { fprintf(stderr, "sift_batch_driver: cloud %zu: keypoint counts differ\n", c); return 1; }
            keypoints += one;
            snapped += snap_batch[c]->size();
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "sift_batch_driver: %s\n", e.what());
        return 1;
    }
    if (!write_result(std::string(argv[1]) + ".batch", kp_batch, snap_batch) || !write_result(std::string(argv[1]) + ".loop", kp_loop, snap_loop)) {
        fprintf(stderr, "sift_batch_driver: cannot write %s.*\n", argv[1]);
        return 2;
    }
    printf("sift_batch_driver clouds=%zu keypoints=%zu snapped=%zu\n", clouds.size(), keypoints, snapped);
    return 0;
}
