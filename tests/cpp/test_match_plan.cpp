// test_match_plan.cpp -- csrc/match_plan.hpp on the CPU (no library, no GPU): the one plan behind pcc_match_knn_batch,
// pcc_match_knn_batch_dims and pcc_cluster_matching.
//   1. frozen tables: match_dims_plan() and cm_layout() reproduce, word for word, what they built before they shared a planner
//      (tests/golden/match_plan_tables.txt)
//   2. the 3-D plan: what match_knn_batch() calls builds the frozen dp = 4 tables for the same pairs
//   3. the pieces by themselves: empty pairs contribute nothing, the widest pairs come first and equal ones keep their order,
//      query blocks are the outer loop, the slice rule's two ends
//   4. 2^31 records or items are refused without an allocation for them
//
// The golden file was written by this program, built with -DMATCH_PLAN_RECORD against the headers of the commit before
// match_plan.hpp existed (match_dims_plan.hpp and cluster_match_plan.hpp each with a planner of its own):
//   g++ -std=c++17 -DMATCH_PLAN_RECORD -Ipointcloudcomparator_amd/csrc tests/cpp/test_match_plan.cpp -o record
//   ./record tests/golden/match_plan_tables.txt
// A record build uses nothing of match_plan.hpp; sections 2 to 4 are not part of it.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "cluster_match_plan.hpp"

using namespace pcc;

static int failures = 0;
#define REQUIRE(c)                                                                  \
    do {                                                                            \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

// ---- the inputs ------------------------------------------------------------------------------------------------------------------
// test_match_dims_plan.cpp's shapes: pair p shares the cloud of pair shares[p] (same pointer AND length), or has its own
struct DimsShape {
    std::vector<size_t> n1, n2;
    std::vector<int> shares;
};
static std::vector<DimsShape> dims_shapes() {
    return {{{1, 15, 16, 17, 255, 257, 2049, 0, 300, 2049}, {1, 63, 64, 65, 130, 1, 64, 5, 0, 129}, {-1, -1, -1, -1, -1, -1, -1, -1, -1, 6}},
            {{}, {}, {}},
            {{0}, {0}, {-1}},
            {{23528, 23528, 5000}, {26308, 700, 4000}, {-1, 0, -1}}};
}
// descriptor counts per cluster of either scene, candidates and states per (i, k)
struct ClusterShape {
    std::vector<size_t> n1s, n2s;
    std::vector<int32_t> cand, state;
    int dp;
};
static std::vector<ClusterShape> cluster_shapes() {
    // one scene-2 cluster the candidate of several scene-1 clusters; a cluster of scene 1 that takes part in nothing
    const ClusterShape few{{4, 255, 256, 257, 513, 9}, {129, 65, 4}, {0, 1, -1,  0, 2, 1,  0, -1, -1,  1, 2, 0,  2, 0, 1,  0, 1, 2},
                           {3, 3, 0,  3, 1, 2,  3, 0, 0,  3, 3, 2,  3, 3, 3,  1, 2, 2}, 4};
    // many wide pairs: the slice at its maximum; widths that differ, so that the order of the pairs matters
    ClusterShape many{{}, {640, 700, 64}, {}, {}, 8};
    for (size_t i = 0; i < 60; ++i) {
        many.n1s.push_back(5000 - 7 * (i % 5));
        many.cand.insert(many.cand.end(), {0, 1, 2});
        many.state.insert(many.state.end(), {3, i % 3 ? 3 : 2, 3});
    }
    ClusterShape few32 = few, many32 = many;
    few32.dp = many32.dp = 32;
    return {few, few32, many, many32};
}

// ---- the tables as text ----------------------------------------------------------------------------------------------------------
struct Fnv {
    uint64_t h = 0xcbf29ce484222325ull;
    void word(uint32_t w) {
        for (int b = 0; b < 4; ++b) { h ^= (w >> (8 * b)) & 0xffu; h *= 0x100000001b3ull; }
    }
};
constexpr size_t ITEMS_IN_FULL = 1024;  // longer tables are recorded by their length and the FNV-1a hash of their words

template <class T>
static void row(std::ostringstream& o, const char* name, const std::vector<T>& v) {
    o << name;
    for (const T& x : v) o << ' ' << x;
    o << '\n';
}

template <class Planner>
static std::string dims_section(size_t shape, int dp, Planner planner) {
    const DimsShape s = dims_shapes()[shape];
    static char arena[1 << 12];
    std::vector<const void*> des1(s.n1.size());
    for (size_t p = 0; p < des1.size(); ++p) des1[p] = arena + (s.shares[p] >= 0 ? s.shares[p] : (int)p) * 64;
    MatchDimsPlan pl;
    std::ostringstream o;
    o << "dims shape " << shape << " dp " << dp << '\n';
    if (!planner(des1.size(), des1.data(), s.n1.data(), s.n2.data(), dp, &pl)) { o << "refused\n"; return o.str(); }
    Fnv f;
    for (const auto& it : pl.items)
        for (uint32_t w : {it.q0, it.nq, it.r0, it.nr, it.ridx0, it.qslot0, it.pad0, it.pad1}) f.word(w);
    o << "slice " << pl.slice << " n_rec " << pl.n_rec << " n_slots " << pl.n_slots << " clouds " << pl.clouds.size() << " items " << pl.items.size()
      << " fnv " << std::hex << f.h << std::dec << '\n';
    std::vector<size_t> cn, crec0;
    for (const auto& c : pl.clouds) { cn.push_back(c.n); crec0.push_back(c.rec0); }
    row(o, "cloud_n", cn);
    row(o, "cloud_rec0", crec0);
    row(o, "cloud_of", pl.cloud_of);
    row(o, "q_rec0", pl.q_rec0);
    row(o, "q_slot0", pl.q_slot0);
    if (pl.items.size() <= ITEMS_IN_FULL)
        for (const auto& it : pl.items)
            o << "item " << it.q0 << ' ' << it.nq << ' ' << it.r0 << ' ' << it.nr << ' ' << it.ridx0 << ' ' << it.qslot0 << ' ' << it.pad0 << ' ' << it.pad1 << '\n';
    return o.str();
}

// (the items by the seven fields they had before they became MatchItem: q0 nq r0 nr qslot0 pad0 pad1)
static std::string cluster_section(size_t shape) {
    const ClusterShape s = cluster_shapes()[shape];
    const size_t nc1 = s.n1s.size(), nc2 = s.n2s.size();
    std::vector<size_t> off1(nc1 + 1, 5), off2(nc2 + 1, 7);  // (offsets need not start at 0)
    for (size_t c = 0; c < nc1; ++c) off1[c + 1] = off1[c] + s.n1s[c];
    for (size_t c = 0; c < nc2; ++c) off2[c + 1] = off2[c] + s.n2s[c];
    ClusterMatchLayout L;
    std::ostringstream o;
    o << "cluster shape " << shape << " dp " << s.dp << '\n';
    if (!cm_layout(s.cand.data(), s.state.data(), nc1, nc2, off1.data(), off2.data(), s.dp, &L)) { o << "refused\n"; return o.str(); }
    Fnv f;
    for (const auto& it : L.items)
        for (uint32_t w : {it.q0, it.nq, it.r0, it.nr, it.qslot0, it.pad0, it.pad1}) f.word(w);
    o << "slice " << L.slice << " n_rec " << L.n_rec << " n_slots " << L.n_slots << " clouds " << L.clouds.size() << " pairs " << L.pairs.size()
      << " items " << L.items.size() << " fnv " << std::hex << f.h << std::dec << '\n';
    for (const auto& c : L.clouds) o << "cloud " << c.rec0 << ' ' << c.n << ' ' << c.side << ' ' << c.pad << ' ' << c.src0 << '\n';
    for (const auto& p : L.pairs) o << "pair " << p.slot0 << ' ' << p.nq << ' ' << p.out << ' ' << p.pad << '\n';
    if (L.items.size() <= ITEMS_IN_FULL)
        for (const auto& it : L.items)
            o << "item " << it.q0 << ' ' << it.nq << ' ' << it.r0 << ' ' << it.nr << ' ' << it.qslot0 << ' ' << it.pad0 << ' ' << it.pad1 << '\n';
    return o.str();
}

static const int DPS[] = {4, 8, 16, 32};

#ifdef MATCH_PLAN_RECORD
int main(int argc, char** argv) {
    std::ofstream out(argc > 1 ? argv[1] : "tests/golden/match_plan_tables.txt");
    out << "# The tables of match_dims_plan() and cm_layout() for the inputs of tests/cpp/test_match_plan.cpp, written by that program\n"
           "# built with -DMATCH_PLAN_RECORD against the headers of the commit before match_plan.hpp existed (see its header).\n"
           "# dims: item = q0 nq r0 nr ridx0 qslot0 pad0 pad1; cluster: cloud = rec0 n side pad src0, pair = slot0 nq out pad,\n"
           "# item = q0 nq r0 nr qslot0 pad0 pad1.  Tables above 1024 items: their length and the FNV-1a hash of their words only.\n";
    for (size_t s = 0; s < dims_shapes().size(); ++s)
        for (int dp : DPS) out << dims_section(s, dp, match_dims_plan);
    for (size_t s = 0; s < cluster_shapes().size(); ++s) out << cluster_section(s);
    return out.good() && !failures ? 0 : 1;
}
#else
#include "match_plan.hpp"

// the golden file cut into its sections (a section starts at a line "dims ..." or "cluster ...")
static std::vector<std::string> golden_sections(const char* path) {
    std::ifstream in(path);
    std::vector<std::string> sections;
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        if (line.rfind("dims ", 0) == 0 || line.rfind("cluster ", 0) == 0) sections.emplace_back();
        if (sections.empty()) return {};
        sections.back() += line + '\n';
    }
    return sections;
}

static void test_frozen_tables(const char* path) {
    const std::vector<std::string> golden = golden_sections(path);
    const size_t n_dims = dims_shapes().size() * 4, n_cluster = cluster_shapes().size();
    REQUIRE(golden.size() == n_dims + n_cluster);
    if (golden.size() != n_dims + n_cluster) return;
    // what match_knn_batch() calls: match_plan() at the 3-D slice maximum
    auto plan_3d = [](size_t n_pairs, const void* const* des1, const size_t* n1, const size_t* n2, int, MatchPlan* pl) {
        return match_plan(n_pairs, des1, n1, n2, match_slice_max_3d(), pl);
    };
    for (size_t s = 0; s < dims_shapes().size(); ++s)
        for (int k = 0; k < 4; ++k) {
            const bool same = dims_section(s, DPS[k], match_dims_plan) == golden[4 * s + k];
            if (!same) std::printf("dims shape %zu dp %d differs from %s\n", s, DPS[k], path);
            REQUIRE(same);
            if (DPS[k] == 4) REQUIRE(dims_section(s, 4, plan_3d) == golden[4 * s + k]);
        }
    for (size_t s = 0; s < n_cluster; ++s) {
        const bool same = cluster_section(s) == golden[n_dims + s];
        if (!same) std::printf("cluster shape %zu differs from %s\n", s, path);
        REQUIRE(same);
    }
    // the inputs are what they are meant to be: a long table (hash alone) and short ones (in full), both slice ends
    REQUIRE(golden[4 * 3 + 3].find("slice 512 ") != std::string::npos && golden[4 * 3 + 3].find("item ") == std::string::npos);
    REQUIRE(golden[0].find("slice 256 ") != std::string::npos && golden[0].find("item ") != std::string::npos);
    REQUIRE(golden[n_dims].find("slice 256 ") != std::string::npos && golden[n_dims + 2].find("slice 2048 ") != std::string::npos);
}

static void test_pieces() {
    // (q_rec0, nq, r_rec0, nr, slot0): an empty query side, an empty reference side, two pairs of equal width around a wider one
    const std::vector<MatchPair> pairs = {{100, 0, 0, 50, 0}, {100, 70, 0, 300, 0}, {170, 5, 0, 0, 70}, {175, 65, 300, 600, 75}, {240, 1, 0, 300, 140}};
    REQUIRE(match_items_at(pairs, 256) == 2 * 2 + 2 * 3 + 1 * 2 && match_items_at(pairs, 2048) == 2 + 2 + 1);
    REQUIRE(match_slice(pairs, 2048) == MATCH_SLICE_MIN && match_slice(pairs, 512) == MATCH_SLICE_MIN);
    std::vector<MatchItem> items;
    REQUIRE(match_items(pairs, 256, &items) && items.size() == 12);
    // the 600-wide pair first: query blocks outside, slices inside; then the two 300-wide pairs in the order given
    const uint32_t want[12][6] = {{175, 64, 300, 256, 0, 75},   {175, 64, 556, 256, 256, 75},  {175, 64, 812, 88, 512, 75},
                                  {239, 1, 300, 256, 0, 139},   {239, 1, 556, 256, 256, 139},  {239, 1, 812, 88, 512, 139},
                                  {100, 64, 0, 256, 0, 0},      {100, 64, 256, 44, 256, 0},    {164, 6, 0, 256, 0, 64},
                                  {164, 6, 256, 44, 256, 64},   {240, 1, 0, 256, 0, 140},      {240, 1, 256, 44, 256, 140}};
    for (size_t k = 0; k < items.size() && k < 12; ++k) {
        const MatchItem& it = items[k];
        REQUIRE(it.q0 == want[k][0] && it.nq == want[k][1] && it.r0 == want[k][2] && it.nr == want[k][3] && it.ridx0 == want[k][4] &&
                it.qslot0 == want[k][5] && it.pad0 == 0 && it.pad1 == 0);
    }
    // the slice rule's other end: 1024 items at the maximum keep it, one fewer halves it
    const std::vector<MatchPair> full = {{0, 64 * 512, 0, 2049, 0}}, short_of = {{0, 64 * 512 - 64, 0, 2049, 0}};
    REQUIRE(match_items_at(full, 2048) == 1024 && match_slice(full, 2048) == 2048 && match_slice(short_of, 2048) == 1024);
    // the shapes the GPU test sends through the 3-D entry: 255, 256 and 257 references fall to the minimum, where 257 are a full
    // slice and a slice of ONE; the fourth pair names the third's cloud, which is laid out once
    {
        static char arena[64];
        const void* des1[4] = {arena, arena + 8, arena + 16, arena + 16};
        const size_t n1[4] = {255, 256, 257, 257}, n2[4] = {63, 64, 65, 70};
        MatchPlan pl;
        REQUIRE(match_plan(4, des1, n1, n2, match_slice_max_3d(), &pl) && pl.slice == MATCH_SLICE_MIN && pl.clouds.size() == 3);
        REQUIRE(pl.n_rec == 255 + 256 + 257 + 63 + 64 + 65 + 70 && pl.cloud_of[3] == 2 && pl.items.size() == 1 + 1 + 2 * 2 + 2 * 2);
        size_t ones = 0;
        for (const MatchItem& it : pl.items) ones += it.nr == 1 && it.ridx0 == 256 && it.r0 == pl.clouds[2].rec0 + 256;
        REQUIRE(ones == 4);
    }
    REQUIRE(match_slice({}, 2048) == MATCH_SLICE_MIN && match_items({}, 256, &items) && items.empty());
    REQUIRE(match_slice_max_3d() == 2048 && match_dims_slice_max(8) == 2048 && match_dims_slice_max(16) == 1024 && match_dims_slice_max(32) == 512);
    static_assert(sizeof(MatchItem) == 32, "the kernels load an item as eight words");
}

static void test_refusals() {
    static char arena[64];
    const void* des1[2] = {arena, arena + 4};
    MatchPlan pl;
    {  // 2^31 records
        const size_t n1[2] = {(size_t)1 << 30, (size_t)1 << 30}, n2[2] = {1, 1};
        REQUIRE(!match_plan(2, des1, n1, n2, match_slice_max_3d(), &pl) && pl.items.capacity() == 0);
        REQUIRE(!match_dims_plan(2, des1, n1, n2, 32, &pl) && pl.items.capacity() == 0);
    }
    {  // 2^30 records, 2^41 items at the widest slice
        const size_t n1[1] = {(size_t)1 << 29}, n2[1] = {(size_t)1 << 29};
        REQUIRE(!match_plan(1, des1, n1, n2, match_slice_max_3d(), &pl) && pl.items.capacity() == 0 && pl.slice == 2048);
        std::vector<MatchItem> items;
        REQUIRE(!match_items({{0, (size_t)1 << 29, 0, (size_t)1 << 29, 0}}, 2048, &items) && items.capacity() == 0);
        const size_t off[2] = {0, (size_t)1 << 29};
        const int32_t cand[3] = {0, -1, -1}, state[3] = {CM_SEARCHED, CM_NONE, CM_NONE};
        ClusterMatchLayout L;
        REQUIRE(!cm_layout(cand, state, 1, 1, off, off, 4, &L) && L.items.capacity() == 0);
    }
    {  // just below: 2^31 - 1 records in 1 item ... is fine (nothing but the tables is allocated)
        const size_t n1[1] = {3}, n2[1] = {4};
        REQUIRE(match_plan(1, des1, n1, n2, match_slice_max_3d(), &pl) && pl.items.size() == 1 && pl.n_rec == 7);
    }
}

int main(int argc, char** argv) {
    test_frozen_tables(argc > 1 ? argv[1] : "tests/golden/match_plan_tables.txt");
    test_pieces();
    test_refusals();
    if (failures) { std::printf("test_match_plan: %d failure(s)\n", failures); return 1; }
    std::printf("test_match_plan: ok\n");
    return 0;
}
#endif
