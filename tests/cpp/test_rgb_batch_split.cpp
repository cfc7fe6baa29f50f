// test_rgb_batch_split.cpp -- the host half of pcc_region_growing_rgb_batch (csrc/rgb_batch_split.hpp), CPU only: the segment
// records and pair lists of several clouds, built as tests/cpp/test_rgb_merge.cpp builds them (rows from orc_kdtree_knn, the
// segments by PCL's queue, the deduplicated pair list by plain host loops), concatenated with the ids of cloud c behind those of
// the clouds before it and the pairs of all clouds shuffled into one list.  The split must give every cloud the
// cluster_of_segment and the cluster count of rgb_merge_regions on that cloud alone, and through them the oracle's labels
// (orc_region_growing_rgb fed the same rows).  Clouds with one segment, with no pair and with no segment at all (a cloud without
// a finite point) sit in the middle.  Built plain and under ASan + UBSan (make test-rgb-batch-split).
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
#include "rgb_batch_split.hpp"

namespace {

struct Scene {
    const char* name;
    size_t n;        // 0: a cloud without a finite point -- no segment
    int colours;     // levels per channel
    int step;        // grey levels between them (0: 256 random levels)
};

struct Cloud {
    std::vector<pcc::RgbSegment> segs;
    std::vector<pcc::RgbSegmentPair> pairs;
    std::vector<int> seg;        // segment of every point
    std::vector<int32_t> want;   // the oracle's labels
    int want_n = 0;
};

constexpr float P2P = 6.f, R2R = 5.f;

bool build(const Scene& sc, float distance, int min_size, int nn, int region_nn, std::mt19937& rng, Cloud* out) {
    const size_t n = sc.n;
    if (n == 0) return true;
    std::uniform_real_distribution<float> uni(0.f, 1.f);
    std::vector<float> pts(n * 3);
    std::vector<uint8_t> rgb(n * 3);
    for (float& v : pts) v = uni(rng);
    for (uint8_t& c : rgb) c = (uint8_t)(sc.step ? (rng() % (unsigned)sc.colours) * (unsigned)sc.step : rng() % 256u);
    const int K = (int)std::min<size_t>((size_t)region_nn, n);
    std::vector<int32_t> nbr(n * (size_t)K, -1);
    std::vector<float> nd2(n * (size_t)K, 0.f);
    orc_kdtree* tree = orc_kdtree_build(pts.data(), n, 12);
    if (!tree) return false;
    for (size_t i = 0; i < n; ++i) orc_kdtree_knn(tree, &pts[i * 3], K, &nbr[i * (size_t)K], &nd2[i * (size_t)K]);
    orc_kdtree_free(tree);
    out->want.assign(n, -1);
    out->want_n = orc_region_growing_rgb(pts.data(), n, 12, rgb.data(), nbr.data(), nd2.data(), K, distance, P2P, R2R, min_size, 0x7fffffff, nn,
                                         region_nn, out->want.data());
    // the segments: seeds in index order, breadth first over the first nn row entries
    std::vector<int>& seg = out->seg;
    seg.assign(n, -1);
    const float p2p2 = P2P * P2P;
    for (size_t s0 = 0; s0 < n; ++s0) {
        if (seg[s0] != -1) continue;
        const int id = (int)out->segs.size();
        std::vector<int> queue(1, (int)s0);
        seg[s0] = id;
        for (size_t head = 0; head < queue.size(); ++head) {
            const int cur = queue[head];
            for (int j = 0; j < nn && j < K; ++j) {
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
        out->segs.push_back(pcc::RgbSegment{0, 0, 0, 0});
    }
    for (size_t i = 0; i < n; ++i) {
        pcc::RgbSegment& r = out->segs[(size_t)seg[i]];
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
    for (const auto& e : best) out->pairs.push_back(pcc::RgbSegmentPair{e.first.first, e.first.second, e.second});
    return true;
}

int run(const char* what, const std::vector<Scene>& scenes, float distance, int min_size, int nn, int region_nn, unsigned seed) {
    std::mt19937 rng(seed);
    const size_t nc = scenes.size();
    std::vector<Cloud> clouds(nc);
    for (size_t c = 0; c < nc; ++c)
        if (!build(scenes[c], distance, min_size, nn, region_nn, rng, &clouds[c])) return 1;
    // every cloud alone
    std::vector<std::vector<int32_t>> alone(nc);
    std::vector<int> alone_n(nc);
    int failed = 0;
    for (size_t c = 0; c < nc; ++c) {
        std::vector<pcc::RgbSegmentPair> pairs = clouds[c].pairs;
        std::shuffle(pairs.begin(), pairs.end(), rng);
        alone_n[c] = pcc::rgb_merge_regions(clouds[c].segs.data(), clouds[c].segs.size(), pairs.data(), pairs.size(), distance * distance, R2R * R2R,
                                            (unsigned int)region_nn, min_size, 0x7fffffff, alone[c]);
        size_t bad = 0;
        for (size_t i = 0; i < clouds[c].seg.size(); ++i) bad += alone[c][(size_t)clouds[c].seg[i]] != clouds[c].want[i];
        if (bad || alone_n[c] != clouds[c].want_n) {
            std::printf("%s cloud %zu (%s): alone %d clusters, oracle %d, %zu labels differ\n", what, c, scenes[c].name, alone_n[c], clouds[c].want_n, bad);
            ++failed;
        }
    }
    // the concatenation: ids of cloud c behind those of the clouds before it, one shuffled pair list
    std::vector<uint32_t> id_base(nc + 1, 0);
    std::vector<pcc::RgbSegment> segs;
    std::vector<pcc::RgbSegmentPair> pairs;
    for (size_t c = 0; c < nc; ++c) {
        const uint32_t b = id_base[c];
        segs.insert(segs.end(), clouds[c].segs.begin(), clouds[c].segs.end());
        for (const pcc::RgbSegmentPair& p : clouds[c].pairs) pairs.push_back(pcc::RgbSegmentPair{p.s + b, p.t + b, p.d2});
        id_base[c + 1] = b + (uint32_t)clouds[c].segs.size();
    }
    std::shuffle(pairs.begin(), pairs.end(), rng);
    std::vector<int32_t> of_segment;
    std::vector<int32_t> ncl(nc, -7);
    const bool ok = pcc::rgb_batch_split(segs.data(), segs.size(), pairs.data(), pairs.size(), id_base.data(), nc, distance * distance, R2R * R2R,
                                         (unsigned int)region_nn, min_size, 0x7fffffff, of_segment, ncl.data());
    if (!ok || of_segment.size() != segs.size()) {
        std::printf("%s: the split refused a well-formed batch\n", what);
        return failed + 1;
    }
    size_t one_segment = 0, no_pair = 0, no_segment = 0;
    for (size_t c = 0; c < nc; ++c) {
        one_segment += clouds[c].segs.size() == 1;
        no_pair += !clouds[c].segs.empty() && clouds[c].pairs.empty();
        no_segment += clouds[c].segs.empty();
        bool same = ncl[c] == alone_n[c];
        for (size_t s = 0; s < clouds[c].segs.size(); ++s) same = same && of_segment[id_base[c] + s] == alone[c][s];
        if (!same) {
            std::printf("%s cloud %zu (%s): the split differs from the cloud alone (%d against %d clusters)\n", what, c, scenes[c].name, ncl[c], alone_n[c]);
            ++failed;
        }
    }
    // a pair that leads from one cloud into another must be refused, wherever it sorts
    if (nc >= 2 && id_base[1] > 0 && id_base[nc] > id_base[1]) {
        std::vector<pcc::RgbSegmentPair> crossing = pairs;
        crossing.push_back(pcc::RgbSegmentPair{0u, id_base[nc] - 1u, 0.25f});
        std::vector<int32_t> tmp_ncl(nc, 0);
        if (pcc::rgb_batch_split(segs.data(), segs.size(), crossing.data(), crossing.size(), id_base.data(), nc, distance * distance, R2R * R2R,
                                 (unsigned int)region_nn, min_size, 0x7fffffff, of_segment, tmp_ncl.data())) {
            std::printf("%s: a pair between two clouds was accepted\n", what);
            ++failed;
        }
    }
    std::printf("%-12s seed %u: %zu clouds, %zu segments, %zu pairs; %zu clouds of one segment, %zu without a pair, %zu without a segment\n", what, seed, nc,
                segs.size(), pairs.size(), one_segment, no_pair, no_segment);
    return failed;
}

}  // namespace

int main() {
    // ("flat": one colour level -- every point joins the first seed: one segment, no pair; "empty": no finite point)
    const std::vector<Scene> mixed = {{"few", 1500, 3, 20}, {"flat", 300, 1, 20}, {"empty", 0, 1, 20}, {"noise", 800, 0, 0},
                                      {"one", 1, 2, 50},    {"empty", 0, 1, 20},  {"tiny", 20, 2, 50}, {"few", 900, 3, 20}};
    const std::vector<Scene> ends = {{"empty", 0, 1, 20}, {"few", 600, 3, 20}, {"flat", 150, 1, 20}, {"empty", 0, 1, 20}};
    const std::vector<Scene> lone = {{"noise", 500, 0, 0}};
    const std::vector<Scene> none = {{"empty", 0, 1, 20}, {"empty", 0, 1, 20}};
    int failed = 0;
    for (unsigned seed = 1; seed <= 2; ++seed) {
        failed += run("mixed-min1", mixed, 10.f, 1, 30, 100, seed);
        failed += run("mixed-min7", mixed, 10.f, 7, 30, 100, seed);
        failed += run("mixed-min200", mixed, 10.f, 200, 30, 100, seed);
        failed += run("mixed-near", mixed, 0.05f, 30, 30, 100, seed);
        failed += run("mixed-nn3", mixed, 10.f, 7, 30, 3, seed);
        failed += run("ends", ends, 10.f, 7, 30, 100, seed);
        failed += run("lone", lone, 10.f, 7, 30, 100, seed);
        failed += run("none", none, 10.f, 7, 30, 100, seed);
    }
    // no cloud at all, and id ranges that do not tile the segments
    std::vector<int32_t> of_segment;
    int32_t ncl[2] = {0, 0};
    if (!pcc::rgb_batch_split(nullptr, 0, nullptr, 0, nullptr, 0, 1.f, 1.f, 100u, 1, 0x7fffffff, of_segment, ncl)) { std::printf("no cloud: refused\n"); ++failed; }
    const pcc::RgbSegment two[2] = {{3, 30, 30, 30}, {4, 40, 40, 40}};
    const uint32_t short_base[3] = {0, 1, 1}, late_base[3] = {1, 1, 2};
    if (pcc::rgb_batch_split(two, 2, nullptr, 0, short_base, 2, 1.f, 1.f, 100u, 1, 0x7fffffff, of_segment, ncl)) { std::printf("short id ranges accepted\n"); ++failed; }
    if (pcc::rgb_batch_split(two, 2, nullptr, 0, late_base, 2, 1.f, 1.f, 100u, 1, 0x7fffffff, of_segment, ncl)) { std::printf("late id ranges accepted\n"); ++failed; }
    if (failed) { std::printf("rgb batch split FAILED (%d)\n", failed); return 1; }
    std::printf("rgb batch split ok\n");
    return 0;
}
