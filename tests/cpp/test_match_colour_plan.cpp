// test_match_colour_plan.cpp -- csrc/match_colour_plan.hpp on the CPU (no library, no GPU): which clusters
// pcc_match_colour_elements segments, in which order and on which route, and the way back to the table.
//   1. first-use order: (i, scene 1) before (i, scene 2), i ascending; rows without a match list nothing
//   2. one entry per distinct cluster when a scene-2 cluster is named by several matches, and the count of what that saved
//   3. the map from (i, side) back to the list, and mc_fill over it
//   4. empty clusters: on the batch route with no point and no item, sharing their base with the next cloud
//   5. the brute limit: a cluster exactly at it stays on the batch route, one above it takes the work handle; limit 0 sends every
//      cluster that holds a record to the work handle
//   6. bases: the prefix sums of the batch clouds, summing to the points on the batch route; the items are rift_batch_plan's
//   7. 2^31 points on the batch route are refused
#include <cstdio>
#include <vector>
#include "match_colour_plan.hpp"

using namespace pcc;

static int failures = 0;
#define REQUIRE(c)                                                                  \
    do {                                                                            \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static std::vector<size_t> offsets_of(const std::vector<size_t>& n, size_t first = 0) {
    std::vector<size_t> o(1, first);
    for (size_t v : n) o.push_back(o.back() + v);
    return o;
}

// what every plan has to satisfy, whatever its inputs
static void check_invariants(const MatchColourPlan& P, const std::vector<int32_t>& matches, const std::vector<size_t>& o1, const std::vector<size_t>& o2,
                             size_t limit) {
    const size_t n1 = matches.size();
    REQUIRE(P.entry.size() == 2 * n1);
    size_t named = 0, batch_points = 0, work_points = 0, n_batch = 0, n_work = 0;
    for (size_t i = 0; i < n1; ++i) {
        if (matches[i] < 0) { REQUIRE(P.entry[2 * i] == -1 && P.entry[2 * i + 1] == -1); continue; }
        named += 2;
        for (int side = 0; side < 2; ++side) {
            const int32_t e = P.entry[2 * i + side];
            REQUIRE(e >= 0 && (size_t)e < P.clusters.size());
            if (e < 0) continue;
            const MatchColourCluster& m = P.clusters[(size_t)e];
            const size_t c = side ? (size_t)matches[i] : i;
            const std::vector<size_t>& o = side ? o2 : o1;
            REQUIRE(m.scene == (uint32_t)side && m.cluster == c && m.src0 == o[c] && m.n == o[c + 1] - o[c]);
        }
    }
    REQUIRE(named == P.clusters.size() + P.n_saved);
    for (size_t e = 0; e < P.clusters.size(); ++e) {
        const MatchColourCluster& m = P.clusters[e];
        for (size_t f = 0; f < e; ++f) REQUIRE(!(P.clusters[f].scene == m.scene && P.clusters[f].cluster == m.cluster));  // distinct
        REQUIRE(m.route == (m.n > limit ? (uint32_t)MC_WORK : (uint32_t)MC_BATCH));
        if (m.route == MC_BATCH) {
            REQUIRE(m.slot == n_batch && m.slot < P.batch_n.size() && P.batch_n[m.slot] == m.n);
            REQUIRE(m.base == P.bases[m.slot] && m.base == batch_points);
            batch_points += m.n;
            ++n_batch;
        } else {
            REQUIRE(m.slot == n_work && m.base == 0);
            work_points += m.n;
            ++n_work;
        }
    }
    REQUIRE(n_batch == P.batch_n.size() && n_work == P.n_work);
    REQUIRE(P.bases.size() == n_batch + 1 && P.bases[0] == 0 && P.bases[n_batch] == batch_points);
    REQUIRE(batch_points == P.n_batch_points && work_points == P.n_work_points);
    // the items are rift_batch_plan's over the batch clouds: every point a query of exactly one item of its own cloud
    std::vector<uint32_t> bases;
    std::vector<RiftBatchItem> items;
    rift_batch_plan(P.batch_n.data(), P.batch_n.size(), &bases, &items);
    REQUIRE(bases == P.bases && items.size() == P.items.size());
    std::vector<int> hit(batch_points, 0);
    for (size_t k = 0; k < P.items.size() && k < items.size(); ++k) {
        const RiftBatchItem& it = P.items[k];
        REQUIRE(it.base == items[k].base && it.n == items[k].n && it.q0 == items[k].q0 && it.nq == items[k].nq);
        REQUIRE(it.q0 + it.nq <= it.n && (size_t)it.base + it.n <= batch_points);
        for (uint32_t q = 0; q < it.nq; ++q) ++hit[it.base + it.q0 + q];
    }
    for (int h : hit) REQUIRE(h == 1);
}

static void test_order_and_deduplication() {
    // scene 1: five clusters; scene 2: four.  Rows 0 and 1 name cluster 2 of scene 2, row 4 cluster 0, rows 2 and 3 nothing
    const std::vector<size_t> o1 = offsets_of({20, 30, 40, 50, 60}, 7), o2 = offsets_of({11, 12, 13, 14}, 3);
    const std::vector<int32_t> matches = {2, 2, -1, -1, 0};
    MatchColourPlan P;
    REQUIRE(mc_plan(matches.data(), 5, o1.data(), 4, o2.data(), 8192, &P));
    check_invariants(P, matches, o1, o2, 8192);
    REQUIRE(P.clusters.size() == 5 && P.n_saved == 1);
    const uint32_t want[5][2] = {{0, 0}, {1, 2}, {0, 1}, {0, 4}, {1, 0}};  // (scene, cluster) in first-use order
    for (size_t e = 0; e < 5 && e < P.clusters.size(); ++e) REQUIRE(P.clusters[e].scene == want[e][0] && P.clusters[e].cluster == want[e][1]);
    const int32_t entry[10] = {0, 1, 2, 1, -1, -1, -1, -1, 3, 4};
    for (size_t k = 0; k < 10; ++k) REQUIRE(P.entry[k] == entry[k]);
    REQUIRE(P.clusters[1].src0 == 3 + 11 + 12 && P.clusters[1].n == 13 && P.clusters[3].src0 == 7 + 20 + 30 + 40 + 50);
    REQUIRE(P.n_batch_points == 20 + 13 + 30 + 60 + 11 && P.n_work == 0 && P.n_work_points == 0);
    // the way back: one count per list entry -> the table
    const int32_t counts[5] = {100, 101, 102, 103, 104};
    int32_t out[10];
    mc_fill(P, counts, 5, out);
    const int32_t table[10] = {100, 101, 102, 101, -1, -1, -1, -1, 103, 104};
    for (size_t k = 0; k < 10; ++k) REQUIRE(out[k] == table[k]);
    // every row names the same cluster of scene 2
    const std::vector<int32_t> all = {3, 3, 3, 3, 3};
    REQUIRE(mc_plan(all.data(), 5, o1.data(), 4, o2.data(), 8192, &P));
    check_invariants(P, all, o1, o2, 8192);
    REQUIRE(P.clusters.size() == 6 && P.n_saved == 4 && P.clusters[1].scene == 1 && P.clusters[1].cluster == 3);
    // no match at all, and no cluster at all
    const std::vector<int32_t> none = {-1, -1, -1, -1, -1};
    REQUIRE(mc_plan(none.data(), 5, o1.data(), 4, o2.data(), 8192, &P));
    check_invariants(P, none, o1, o2, 8192);
    REQUIRE(P.clusters.empty() && P.batch_n.empty() && P.bases.size() == 1 && P.bases[0] == 0 && P.items.empty() && P.n_saved == 0);
    REQUIRE(mc_plan(nullptr, 0, o1.data(), 0, o2.data(), 8192, &P));
    REQUIRE(P.clusters.empty() && P.entry.empty() && P.bases.size() == 1);
}

static void test_empty_clusters() {
    const std::vector<size_t> o1 = offsets_of({5, 0, 7}), o2 = offsets_of({0, 9, 0});
    const std::vector<int32_t> matches = {0, 1, 2};
    MatchColourPlan P;
    REQUIRE(mc_plan(matches.data(), 3, o1.data(), 3, o2.data(), 100, &P));
    check_invariants(P, matches, o1, o2, 100);
    REQUIRE(P.clusters.size() == 6 && P.n_batch_points == 21);
    const uint32_t bases[7] = {0, 5, 5, 5, 14, 21, 21};  // (an empty cloud shares its base with the next one)
    for (size_t k = 0; k < 7; ++k) REQUIRE(P.bases[k] == bases[k]);
    for (const RiftBatchItem& it : P.items) REQUIRE(it.n > 0 && it.nq > 0);
    // nothing but empty clusters: a batch route without a point
    const std::vector<size_t> e1 = offsets_of({0, 0}, 4), e2 = offsets_of({0}, 9);
    const std::vector<int32_t> m2 = {0, 0};
    REQUIRE(mc_plan(m2.data(), 2, e1.data(), 1, e2.data(), 100, &P));
    check_invariants(P, m2, e1, e2, 100);
    REQUIRE(P.clusters.size() == 3 && P.n_saved == 1 && P.n_batch_points == 0 && P.items.empty() && P.n_work == 0);
}

static void test_brute_limit() {
    const std::vector<size_t> o1 = offsets_of({256, 257, 255}), o2 = offsets_of({257, 256, 1, 0});
    const std::vector<int32_t> matches = {0, 1, 3};
    MatchColourPlan P;
    REQUIRE(mc_plan(matches.data(), 3, o1.data(), 4, o2.data(), 256, &P));
    check_invariants(P, matches, o1, o2, 256);
    // list: (0,0) 256 batch, (1,0) 257 work, (0,1) 257 work, (1,1) 256 batch, (0,2) 255 batch, (1,3) 0 batch
    REQUIRE(P.clusters.size() == 6);
    const uint32_t route[6] = {MC_BATCH, MC_WORK, MC_WORK, MC_BATCH, MC_BATCH, MC_BATCH};
    for (size_t e = 0; e < 6 && e < P.clusters.size(); ++e) REQUIRE(P.clusters[e].route == route[e]);
    REQUIRE(P.n_batch_points == 256 + 256 + 255 && P.n_work_points == 2 * 257 && P.n_work == 2 && P.batch_n.size() == 4);
    // limit 0 (nr_region_neighbours > 128): every cluster with a record takes the work handle, the empty one stays
    REQUIRE(mc_plan(matches.data(), 3, o1.data(), 4, o2.data(), 0, &P));
    check_invariants(P, matches, o1, o2, 0);
    REQUIRE(P.n_work == 5 && P.n_batch_points == 0 && P.batch_n.size() == 1 && P.items.empty());
    // a limit above everything
    REQUIRE(mc_plan(matches.data(), 3, o1.data(), 4, o2.data(), (size_t)1 << 40, &P));
    check_invariants(P, matches, o1, o2, (size_t)1 << 40);
    REQUIRE(P.n_work == 0 && P.n_batch_points == 256 + 257 + 257 + 256 + 255);
}

static void test_too_many_points() {
    // two clusters of 2^30 records each on the batch route: 2^31 points (only the offsets are read)
    const std::vector<size_t> o1 = offsets_of({(size_t)1 << 30}), o2 = offsets_of({(size_t)1 << 30});
    const std::vector<int32_t> matches = {0};
    MatchColourPlan P;
    REQUIRE(!mc_plan(matches.data(), 1, o1.data(), 1, o2.data(), (size_t)1 << 31, &P));
    // ... and the same on the work handle is a plan (without an item)
    REQUIRE(mc_plan(matches.data(), 1, o1.data(), 1, o2.data(), 8192, &P));
    REQUIRE(P.n_work == 2 && P.items.empty() && P.n_work_points == (size_t)1 << 31);
}

int main() {
    test_order_and_deduplication();
    test_empty_clusters();
    test_brute_limit();
    test_too_many_points();
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("match_colour_plan: ok\n");
    return 0;
}
