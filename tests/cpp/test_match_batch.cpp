// test_match_batch.cpp -- pcc::matchRIFTFeaturesKnnBatch and the report's cluster matching on top of it (needs a GPU).
//   1. matchRIFTFeaturesKnnBatch(pairs) equals a loop of matchRIFTFeaturesKnn over the same pairs, element for element
//      (tie-laden descriptors, shared first clouds, null and empty clouds, sizes around the workgroup's 64 queries).
//   2. report::clusterSections on two small scenes with descriptors writes the results.txt bytes and the stdout lines
//      recorded in tests/golden/match_batch_report_{results,stdout}.txt.  Those were recorded ONCE with this same program
//      built against the headers of the commit before the batch call (-DPCC_MATCH_BATCH_RECORD: part 1 left out, the files
//      written instead of compared), i.e. they are the output of one matchRIFTFeaturesKnn call per gated pair.
// usage: test_match_batch GOLDEN_DIR        prints "match batch ok"; exit code 77 = no GPU
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include "report.hpp"

using namespace pcc;
#define REQUIRE(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// a generator whose values do not depend on the standard library at hand
struct Lcg {
    uint64_t s;
    explicit Lcg(uint64_t seed) : s(seed * 2862933555777941757ull + 3037000493ull) {}
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    float unit() { return (float)(next() >> 7) * (1.0f / 16777216.0f); }  // 24 bits: exact in a float
};

static std::string slurp(const std::string& p) {
    std::ifstream f(p.c_str(), std::ios::binary);
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

// n records on the 1/64 lattice (duplicates in the three bins the search reads: ties in most queries)
static report::DescPtr lattice(size_t n, uint64_t seed) {
    report::DescPtr d(new PointCloud<RIFT32>);
    Lcg g(seed);
    for (size_t i = 0; i < n; ++i) {
        RIFT32 h;
        for (float& v : h.histogram) v = (float)(g.next() % 9) / 64.0f;
        d->push_back(h);
    }
    return d;
}
// n records taken from `from` (cyclically, starting at `shift`), every `far_every`-th moved out of the threshold's reach
static report::DescPtr taken_from(const report::DescPtr& from, size_t n, size_t shift, size_t far_every) {
    report::DescPtr d(new PointCloud<RIFT32>);
    for (size_t i = 0; i < n; ++i) {
        RIFT32 h = from->points[(i + shift) % from->size()];
        if (far_every && i % far_every == far_every - 1) h.histogram[0] += 1.0f;
        d->push_back(h);
    }
    return d;
}
// a ball of n coloured points
static report::CloudPtr ball(size_t n, float cx, float cy, float cz, uint64_t seed) {
    report::CloudPtr c(new PointCloud<PointXYZRGB>);
    Lcg g(seed);
    for (size_t i = 0; i < n; ++i) {
        PointXYZRGB p;
        p.x = cx + 0.2f * g.unit(); p.y = cy + 0.2f * g.unit(); p.z = cz + 0.2f * g.unit();
        p.r = (uint8_t)(i % 2 ? 200 : 40); p.g = (uint8_t)(g.next() % 30); p.b = (uint8_t)(p.x > cx + 0.1f ? 220 : 20); p.a = 255;
        c->push_back(p);
    }
    return c;
}

struct Scene {
    std::vector<report::CloudPtr> clusters1, clusters2;
    std::vector<report::DescPtr> des1, des2;
};

// scene A: 5 clusters against 6, most of them face to face; descriptor counts on both sides of every gate, matches that are
// accepted with and without the "Match accepted" line, and matches that fail
static Scene scene_a() {
    Scene s;
    const size_t pts1[5] = {300, 340, 380, 420, 260}, pts2[6] = {310, 350, 760, 430, 250, 300};
    const size_t nd1[5] = {40, 66, 3, 130, 25}, nd2[6] = {40, 65, 30, 129, 0, 50};
    for (int i = 0; i < 5; ++i) {
        s.clusters1.push_back(ball(pts1[i], 2.0f * i, 0.f, 0.f, 100 + i));
        s.des1.push_back(lattice(nd1[i], 200 + i));
    }
    for (int j = 0; j < 6; ++j) {
        s.clusters2.push_back(ball(pts2[j], j < 5 ? 2.0f * j + 0.3f : 4.9f, j < 5 ? 0.1f : 1.0f, 0.f, 300 + j));
        if (j < 4 && nd2[j]) s.des2.push_back(taken_from(s.des1[j], nd2[j], j, j == 3 ? 4 : 0));
        else s.des2.push_back(lattice(nd2[j], 400 + j));
    }
    return s;
}
// scene B: 3 clusters against 2 -- the third candidate does not exist ("No closer centroid found")
static Scene scene_b() {
    Scene s;
    const size_t pts1[3] = {280, 500, 300}, pts2[2] = {290, 520};
    for (int i = 0; i < 3; ++i) {
        s.clusters1.push_back(ball(pts1[i], 0.f, 3.0f * i, 1.f, 500 + i));
        s.des1.push_back(lattice(70 + 30 * i, 600 + i));
    }
    for (int j = 0; j < 2; ++j) {
        s.clusters2.push_back(ball(pts2[j], 0.2f, 3.0f * j, 1.f, 700 + j));
        s.des2.push_back(taken_from(s.des1[j], 70 + 30 * j + (j ? 0 : 1), 3, 0));
    }
    return s;
}

int main(int argc, char** argv) {
    int ndev = 0;
    if (pcc_device_count(&ndev) != PCC_OK || ndev == 0) { std::printf("no HIP device: skipped\n"); return 77; }
    const std::string golden = argc > 1 ? argv[1] : "tests/golden";

#ifndef PCC_MATCH_BATCH_RECORD
    {
        std::vector<std::pair<report::DescPtr, report::DescPtr> > pairs;
        const size_t sizes[] = {1, 4, 63, 64, 65, 130, 700, 5000};
        report::DescPtr shared = lattice(300, 9);
        for (size_t a = 0; a < 8; ++a) {
            report::DescPtr d1 = lattice(sizes[a], 10 + a);
            pairs.push_back(std::make_pair(d1, taken_from(d1, sizes[(a + 3) % 8], a, 3)));
            pairs.push_back(std::make_pair(shared, taken_from(shared, sizes[a], a, 5)));
        }
        pairs.push_back(std::make_pair(report::DescPtr(), shared));                              // null / empty clouds: the dummy alone
        pairs.push_back(std::make_pair(shared, report::DescPtr()));
        pairs.push_back(std::make_pair(report::DescPtr(new PointCloud<RIFT32>), shared));
        pairs.push_back(std::make_pair(shared, report::DescPtr(new PointCloud<RIFT32>)));
        const std::vector<std::vector<int> > got = matchRIFTFeaturesKnnBatch(pairs);
        REQUIRE(got.size() == pairs.size());
        size_t matched = 0;
        for (size_t p = 0; p < pairs.size(); ++p) {
            const std::vector<int> want = matchRIFTFeaturesKnn(pairs[p].first, pairs[p].second);
            REQUIRE(got[p] == want);
            REQUIRE(!got[p].empty() && got[p][0] == 0);
            matched += got[p].size() - 1;
        }
        REQUIRE(matched > 1000);
        for (size_t p = pairs.size() - 4; p < pairs.size(); ++p) REQUIRE(got[p].size() == 1);
        REQUIRE(matchRIFTFeaturesKnnBatch(std::vector<std::pair<report::DescPtr, report::DescPtr> >()).empty());
    }
#endif

    // the report's cluster matching on two scenes, stdout captured
    const std::string out_path = "/tmp/pcc_match_batch_results.txt";
    std::ostringstream captured;
    std::streambuf* old = std::cout.rdbuf(captured.rdbuf());
    size_t accepted = 0;
    {
        report::Writer w(out_path);
        Scene scenes[2] = {scene_a(), scene_b()};
        for (Scene& s : scenes) {
            std::vector<int> matches;
            const report::Scores sc = report::clusterSections(w, s.clusters1, s.clusters2, s.des1, s.des2, matches);
            report::scoreSections(w, sc, s.clusters2.size());
            for (int m : matches) accepted += m != -1;
        }
        w.close();
    }
    std::cout.rdbuf(old);
    const std::string results = slurp(out_path), printed = captured.str();
    REQUIRE(accepted >= 3);  // (the scenes really reach the accepted-match sections)
    REQUIRE(printed.find("No closer centroid found") != std::string::npos && printed.find("Match accepted") != std::string::npos);
#ifdef PCC_MATCH_BATCH_RECORD
    { std::ofstream f((golden + "/match_batch_report_results.txt").c_str(), std::ios::binary); f << results; }
    { std::ofstream f((golden + "/match_batch_report_stdout.txt").c_str(), std::ios::binary); f << printed; }
    std::printf("recorded %zu + %zu bytes, %zu accepted matches\n", results.size(), printed.size(), accepted);
#else
    const std::string want_results = slurp(golden + "/match_batch_report_results.txt");
    const std::string want_printed = slurp(golden + "/match_batch_report_stdout.txt");
    REQUIRE(!want_results.empty() && !want_printed.empty());
    REQUIRE(results == want_results);
    REQUIRE(printed == want_printed);
    std::printf("match batch ok\n");
#endif
    return 0;
}
