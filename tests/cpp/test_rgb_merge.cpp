// test_rgb_merge.cpp -- the host half of pcc_region_growing_rgb (csrc/rgb_merge.hpp) against the oracle's restatement of
// pcl::RegionGrowingRGB (orc_region_growing_rgb), CPU only: rows from orc_kdtree_knn, the segments, their records and the
// deduplicated segment pair list by plain host loops (what the kernels of region_rgb.hip hand back), then
// rgb_merge_regions; the labels must be the oracle's, fed the same rows.  Built plain and under ASan + UBSan
// (make test-rgb-merge).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <utility>
#include <vector>

extern "C" {
#include "pcc_oracle.h"
}
#include "rgb_merge.hpp"

namespace {

struct Scene {
    const char* name;
    size_t n;
    int colours;      // levels per channel
    int step;         // grey levels between them (0: 256 random levels)
    float distance;   // distance threshold
    int min_size;
    int nn, region_nn;
};

int run(const Scene& sc, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> uni(0.f, 1.f);
    const size_t n = sc.n;
    std::vector<float> pts(n * 3);
    std::vector<uint8_t> rgb(n * 3);
    for (float& v : pts) v = uni(rng);
    for (uint8_t& c : rgb) c = (uint8_t)(sc.step ? (rng() % (unsigned)sc.colours) * (unsigned)sc.step : rng() % 256u);
    const int K = (int)std::min<size_t>((size_t)sc.region_nn, n);
    std::vector<int32_t> nbr(n * (size_t)K, -1);
    std::vector<float> nd2(n * (size_t)K, 0.f);
    orc_kdtree* tree = orc_kdtree_build(pts.data(), n, 12);
    if (!tree) return 1;
    for (size_t i = 0; i < n; ++i) orc_kdtree_knn(tree, &pts[i * 3], K, &nbr[i * (size_t)K], &nd2[i * (size_t)K]);
    orc_kdtree_free(tree);
    const float p2p = 6.f, r2r = 5.f;
    std::vector<int32_t> want(n, -1);
    const int want_n = orc_region_growing_rgb(pts.data(), n, 12, rgb.data(), nbr.data(), nd2.data(), K, sc.distance, p2p, r2r, sc.min_size,
                                              0x7fffffff, sc.nn, sc.region_nn, want.data());
    // the segments: seeds in index order, breadth first over the first nn row entries
    std::vector<int> seg(n, -1);
    std::vector<pcc::RgbSegment> segs;
    const float p2p2 = p2p * p2p;
    for (size_t s0 = 0; s0 < n; ++s0) {
        if (seg[s0] != -1) continue;
        const int id = (int)segs.size();
        std::vector<int> queue(1, (int)s0);
        seg[s0] = id;
        for (size_t head = 0; head < queue.size(); ++head) {
            const int cur = queue[head];
            for (int j = 0; j < sc.nn && j < K; ++j) {
                const int v = nbr[(size_t)cur * K + j];
                if (v < 0 || seg[(size_t)v] != -1) continue;
                unsigned int diff = 0;
                for (int c = 0; c < 3; ++c) {
                    const int d = (int)rgb[(size_t)cur * 3 + c] - (int)rgb[(size_t)v * 3 + c];
                    diff += (unsigned int)(d * d);
                }
                if ((float)diff > p2p2) continue;
                seg[(size_t)v] = id;
                queue.push_back(v);
            }
        }
        segs.push_back(pcc::RgbSegment{0, 0, 0, 0});
    }
    for (size_t i = 0; i < n; ++i) {
        pcc::RgbSegment& r = segs[(size_t)seg[i]];
        r.size += 1;
        r.sum_r += rgb[i * 3];
        r.sum_g += rgb[i * 3 + 1];
        r.sum_b += rgb[i * 3 + 2];
    }
    // the pair list: min row distance per ordered pair of different segments, over all K entries
    std::map<std::pair<uint32_t, uint32_t>, float> best;
    for (size_t i = 0; i < n; ++i)
        for (int j = 0; j < K; ++j) {
            const int v = nbr[i * (size_t)K + j];
            if (v < 0 || seg[(size_t)v] == seg[i]) continue;
            const std::pair<uint32_t, uint32_t> key((uint32_t)seg[i], (uint32_t)seg[(size_t)v]);
            auto it = best.find(key);
            if (it == best.end()) best[key] = nd2[i * (size_t)K + j];
            else if (it->second > nd2[i * (size_t)K + j]) it->second = nd2[i * (size_t)K + j];
        }
    std::vector<pcc::RgbSegmentPair> pairs;
    for (const auto& e : best) pairs.push_back(pcc::RgbSegmentPair{e.first.first, e.first.second, e.second});
    // (the device hands the list over in no particular order)
    std::shuffle(pairs.begin(), pairs.end(), rng);
    std::vector<int32_t> cluster_of_segment;
    const int got_n = pcc::rgb_merge_regions(segs.data(), segs.size(), pairs.data(), pairs.size(), sc.distance * sc.distance, r2r * r2r,
                                             (unsigned int)sc.region_nn, sc.min_size, 0x7fffffff, cluster_of_segment);
    size_t bad = 0;
    for (size_t i = 0; i < n; ++i) bad += cluster_of_segment[(size_t)seg[i]] != want[i];
    std::printf("%-14s seed %u: %zu points, %zu segments, %zu pairs, clusters %d (oracle %d), %zu labels differ\n", sc.name, seed, n, segs.size(),
                pairs.size(), got_n, want_n, bad);
    return (bad || got_n != want_n) ? 1 : 0;
}

}  // namespace

int main() {
    const Scene scenes[] = {
        {"few-min1", 2000, 3, 20, 10.f, 1, 30, 100},   {"few-min7", 2000, 3, 20, 10.f, 7, 30, 100},
        {"few-min200", 2000, 3, 20, 10.f, 200, 30, 100}, {"noise", 1500, 0, 0, 10.f, 200, 30, 100},
        {"near", 2000, 3, 20, 0.05f, 30, 30, 100},     {"region-nn3", 2000, 3, 20, 10.f, 7, 30, 3},
        {"tiny", 20, 2, 50, 10.f, 5, 30, 100},         {"one", 1, 2, 50, 10.f, 1, 30, 100},
    };
    int failed = 0;
    for (const Scene& sc : scenes)
        for (unsigned seed = 1; seed <= 2; ++seed) failed += run(sc, seed);
    if (failed) { std::printf("rgb merge FAILED (%d)\n", failed); return 1; }
    std::printf("rgb merge ok\n");
    return 0;
}
