// test_cluster_match_plan.cpp -- csrc/cluster_match_plan.hpp on the CPU (no library, no GPU): the decisions of the
// cluster-matching loop and the tables of pcc_cluster_matching's search.
//   1. candidates: three nearest free centroids in order of distance, the lowest index among equal distances, -1 for fewer than
//      three clusters, a NaN centroid and a centroid 2e12 away; the arithmetic (float differences, double squares, float root)
//   2. gates: the descriptor counts first, then the size_t quotient of the point counts; points1 == 0 is gated out
//   3. acceptance: corr / max(n1, n2) >= 1 and corr > best, the earlier of two equal candidates
//   4. the tables: every participating cluster packed once, every query of a pair in exactly one item per slice of its
//      references, every reference of the pair in exactly one slice, slots disjoint, the slice 256 with few pairs
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <set>
#include <vector>
#include "cluster_match_plan.hpp"

using namespace pcc;

static int failures = 0;
#define REQUIRE(c)                                                                  \
    do {                                                                            \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static void test_candidates() {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    // scene 2: 0 and 3 equidistant from the origin, 1 nearer, 2 NaN, 4 too far away
    const float c2[] = {2, 0, 0,  1, 0, 0,  nan, 0, 0,  0, 2, 0,  2e12f, 0, 0,  0, 0, 3};
    const float c1[] = {0, 0, 0,  nan, 0, 0,  0, 0, 2.9f};
    int32_t cand[9];
    cm_candidates(c1, 3, c2, 6, cand);
    REQUIRE(cand[0] == 1 && cand[1] == 0 && cand[2] == 3);     // (0 before 3: the lowest index among equal distances)
    REQUIRE(cand[3] == -1 && cand[4] == -1 && cand[5] == -1);  // a NaN centroid has no candidate
    REQUIRE(cand[6] == 5);
    // 0, 1 and 2 clusters in scene 2
    cm_candidates(c1, 1, c2, 0, cand);
    REQUIRE(cand[0] == -1 && cand[1] == -1 && cand[2] == -1);
    cm_candidates(c1, 1, c2, 1, cand);
    REQUIRE(cand[0] == 0 && cand[1] == -1 && cand[2] == -1);
    cm_candidates(c1, 1, c2, 2, cand);
    REQUIRE(cand[0] == 1 && cand[1] == 0 && cand[2] == -1);
    // only NaN and far centroids left
    const float far2[] = {nan, 0, 0,  2e12f, 0, 0,  1e12f, 0, 0,  9.9e11f, 0, 0};
    cm_candidates(c1, 1, far2, 4, cand);
    REQUIRE(cand[0] == 3 && cand[1] == -1 && cand[2] == -1);   // (1e12 itself is not < 1e12)
    // the arithmetic: squares and their sum in double, rounded to float once, then a float root.  a = 1 + 2^-12: a * a and three
    // times that are exact in double; a centroid along x at exactly that root ties with (a, a, a) -- the lower index wins --,
    // one a float below it comes first
    const float a = 1.0f + 1.0f / 4096.0f;
    const float z[] = {0, 0, 0};
    const float want = std::sqrt((float)(3.0 * ((double)a * (double)a)));
    const float tie2[] = {a, a, a,  want, 0, 0};
    cm_candidates(z, 1, tie2, 2, cand);
    REQUIRE(cand[0] == 0 && cand[1] == 1);
    const float tie3[] = {a, a, a,  std::nextafter(want, 0.0f), 0, 0};
    cm_candidates(z, 1, tie3, 2, cand);
    REQUIRE(cand[0] == 1 && cand[1] == 0);
    const float tie4[] = {a, a, a,  std::nextafter(want, 4.0f), 0, 0};
    cm_candidates(z, 1, tie4, 2, cand);
    REQUIRE(cand[0] == 0 && cand[1] == 1);
}

static void test_states_and_accept() {
    // scene 1: one cluster of 100 points; scene 2: candidates of 99 / 100 / 199 / 200 points, then counts at the gate
    const int32_t cand[] = {0, 1, 2,  3, 4, -1,  0, 1, 2,  1, 1, 1};
    const size_t off1[] = {0, 10, 20, 23, 33};        // descriptor counts 10, 10, 3, 10
    const size_t off2[] = {0, 10, 20, 30, 40, 43};    // 10, 10, 10, 10, 3
    const size_t p1[] = {100, 100, 100, 0}, p2[] = {99, 100, 199, 200, 100};
    int32_t st[12];
    cm_states(cand, 4, off1, off2, p1, p2, st);
    REQUIRE(st[0] == CM_GATED_SIZE && st[1] == CM_SEARCHED && st[2] == CM_SEARCHED);     // 99 / 100 = 0, 100 / 100 = 1, 199 / 100 = 1
    REQUIRE(st[3] == CM_GATED_SIZE && st[4] == CM_GATED_COUNTS && st[5] == CM_NONE);     // 200 / 100 = 2; 3 descriptors; no candidate
    REQUIRE(st[6] == CM_GATED_COUNTS && st[7] == CM_GATED_COUNTS && st[8] == CM_GATED_COUNTS);  // (the counts come first: 99 points too)
    REQUIRE(st[9] == CM_GATED_SIZE && st[10] == CM_GATED_SIZE && st[11] == CM_GATED_SIZE);      // points1 == 0: not divided by

    // acceptance: descriptor counts n1 = 10 against n2 = 10, 9, 8, 12
    const size_t a1[] = {0, 10}, a2[] = {0, 10, 19, 27, 39};
    int32_t m[1];
    auto accept = [&](int32_t j0, uint32_t c0, int32_t j1, uint32_t c1, int32_t j2, uint32_t c2) {
        const int32_t cd[] = {j0, j1, j2};
        const int32_t s3[] = {j0 < 0 ? CM_NONE : CM_SEARCHED, j1 < 0 ? CM_NONE : CM_SEARCHED, j2 < 0 ? CM_NONE : CM_SEARCHED};
        const uint32_t corr[] = {c0, c1, c2};
        cm_accept(cd, s3, corr, 1, a1, a2, m);
        return m[0];
    };
    REQUIRE(accept(0, 10, -1, 0, -1, 0) == 0);    // n1 == n2 = 10: 9 matched + the dummy = 10
    REQUIRE(accept(0, 9, -1, 0, -1, 0) == -1);    // 8 matched: 9 / 10 = 0
    REQUIRE(accept(1, 10, -1, 0, -1, 0) == 1);    // n1 = n2 + 1, all 9 matched: 10 / 10
    REQUIRE(accept(2, 9, -1, 0, -1, 0) == -1);    // n1 = n2 + 2: at most 9 / 10
    REQUIRE(accept(3, 12, -1, 0, -1, 0) == 3);    // n1 < n2 = 12: 11 matched
    REQUIRE(accept(3, 11, -1, 0, -1, 0) == -1);   // 10 matched
    REQUIRE(accept(0, 10, 1, 10, -1, 0) == 0);    // two full candidates with equal corr: the earlier one
    REQUIRE(accept(0, 10, 3, 13, 1, 10) == 3);    // a larger corr replaces it, a smaller one behind does not
    // a state other than searched is skipped whatever its count says
    const int32_t cd[] = {0, 1, 3}, sg[] = {CM_GATED_SIZE, CM_GATED_COUNTS, CM_NONE};
    const uint32_t corr[] = {100, 100, 100};
    cm_accept(cd, sg, corr, 1, a1, a2, m);
    REQUIRE(m[0] == -1);
}

static void check_layout(const std::vector<size_t>& n1s, const std::vector<size_t>& n2s, const std::vector<int32_t>& cand,
                         const std::vector<int32_t>& st, int dp, unsigned int want_slice) {
    const size_t nc1 = n1s.size(), nc2 = n2s.size();
    std::vector<size_t> off1(nc1 + 1, 5), off2(nc2 + 1, 7);  // (offsets need not start at 0)
    for (size_t c = 0; c < nc1; ++c) off1[c + 1] = off1[c] + n1s[c];
    for (size_t c = 0; c < nc2; ++c) off2[c + 1] = off2[c] + n2s[c];
    ClusterMatchLayout L;
    REQUIRE(cm_layout(cand.data(), st.data(), nc1, nc2, off1.data(), off2.data(), dp, &L));
    if (want_slice) REQUIRE(L.slice == want_slice);
    // the clouds: every participating cluster once, back to back
    std::map<std::pair<int, size_t>, const ClusterMatchCloud*> by_src;
    size_t at = 0;
    for (const ClusterMatchCloud& c : L.clouds) {
        REQUIRE(c.rec0 == at && c.n > 0);
        at += c.n;
        REQUIRE(by_src.emplace(std::make_pair((int)c.side, (size_t)c.src0), &c).second);
    }
    REQUIRE(at == L.n_rec);
    // the pairs: in (i, k) order, slots back to back
    size_t n_pairs = 0, slots = 0;
    for (size_t e = 0; e < 3 * nc1; ++e) {
        if (st[e] != CM_SEARCHED) continue;
        REQUIRE(n_pairs < L.pairs.size());
        const ClusterMatchPair& p = L.pairs[n_pairs++];
        REQUIRE(p.out == e && p.slot0 == slots && p.nq == n2s[(size_t)cand[e]]);
        slots += p.nq;
    }
    REQUIRE(n_pairs == L.pairs.size() && slots == L.n_slots);
    // the items: per pair, every (query, reference) exactly once
    std::vector<std::map<std::pair<size_t, size_t>, int> > seen(L.pairs.size());
    for (const MatchItem& it : L.items) {
        REQUIRE(it.nq >= 1 && it.nq <= 64 && it.nr >= 1 && it.nr <= L.slice);
        REQUIRE((size_t)it.q0 + it.nq <= L.n_rec && (size_t)it.r0 + it.nr <= L.n_rec && (size_t)it.qslot0 + it.nq <= L.n_slots);
        size_t p = 0;
        while (p < L.pairs.size() && !(it.qslot0 >= L.pairs[p].slot0 && it.qslot0 < L.pairs[p].slot0 + L.pairs[p].nq)) ++p;
        REQUIRE(p < L.pairs.size());
        if (p == L.pairs.size()) continue;
        const size_t e = L.pairs[p].out, i = e / 3, j = (size_t)cand[e];
        const ClusterMatchCloud* ci = by_src[std::make_pair(0, off1[i])];
        const ClusterMatchCloud* cj = by_src[std::make_pair(1, off2[j])];
        REQUIRE(ci && cj);
        if (!ci || !cj) continue;
        REQUIRE(ci->n == n1s[i] && cj->n == n2s[j]);
        REQUIRE(it.qslot0 + it.nq <= L.pairs[p].slot0 + L.pairs[p].nq);                    // no item across a pair
        REQUIRE(it.q0 - cj->rec0 == it.qslot0 - L.pairs[p].slot0);                         // the slot of a query is its place
        REQUIRE(it.q0 >= cj->rec0 && it.q0 + it.nq <= cj->rec0 + cj->n);
        REQUIRE(it.r0 >= ci->rec0 && it.r0 + it.nr <= ci->rec0 + ci->n);
        REQUIRE((it.q0 - cj->rec0) % 64 == 0 && (it.r0 - ci->rec0) % L.slice == 0);
        ++seen[p][std::make_pair((size_t)(it.q0 - cj->rec0), (size_t)(it.r0 - ci->rec0))];
    }
    for (size_t p = 0; p < L.pairs.size(); ++p) {
        const size_t e = L.pairs[p].out, n1 = n1s[e / 3], n2 = n2s[(size_t)cand[e]];
        REQUIRE(seen[p].size() == ((n2 + 63) / 64) * ((n1 + L.slice - 1) / L.slice));
        for (const auto& kv : seen[p]) REQUIRE(kv.second == 1);
    }
}

static void test_layout() {
    // one scene-2 cluster the candidate of three scene-1 clusters; a cluster of scene 1 that takes part in nothing
    check_layout({4, 255, 256, 257, 513, 9}, {129, 65, 4}, {0, 1, -1,  0, 2, 1,  0, -1, -1,  1, 2, 0,  2, 0, 1,  0, 1, 2},
                 {3, 3, 0,  3, 1, 2,  3, 0, 0,  3, 3, 2,  3, 3, 3,  1, 2, 2}, 4, 256);
    check_layout({4, 255, 256, 257, 513, 9}, {129, 65, 4}, {0, 1, -1,  0, 2, 1,  0, -1, -1,  1, 2, 0,  2, 0, 1,  0, 1, 2},
                 {3, 3, 0,  3, 1, 2,  3, 0, 0,  3, 3, 2,  3, 3, 3,  1, 2, 2}, 32, 256);
    // nothing searched: empty tables
    ClusterMatchLayout L;
    const int32_t cand[] = {0, -1, -1}, st[] = {2, 0, 0};
    const size_t off1[] = {0, 10}, off2[] = {0, 10};
    REQUIRE(cm_layout(cand, st, 1, 1, off1, off2, 4, &L));
    REQUIRE(L.clouds.empty() && L.pairs.empty() && L.items.empty() && L.n_rec == 0 && L.n_slots == 0);
    // many wide pairs: the slice grows to its maximum (2048 at DP <= 8, 512 at DP = 32)
    std::vector<size_t> n1s(400, 5000), n2s(3, 640);
    std::vector<int32_t> cd, ss;
    for (size_t i = 0; i < 400; ++i) { cd.insert(cd.end(), {0, 1, 2}); ss.insert(ss.end(), {3, 3, 3}); }
    check_layout(n1s, n2s, cd, ss, 8, 2048);
    check_layout(n1s, n2s, cd, ss, 32, 512);
    // 2^31 records and more are refused
    const size_t big1[] = {0, (size_t)1 << 30}, big2[] = {0, (size_t)1 << 30};
    const int32_t c0[] = {0, -1, -1}, s0[] = {3, 0, 0};
    REQUIRE(!cm_layout(c0, s0, 1, 1, big1, big2, 4, &L));
}

int main() {
    test_candidates();
    test_states_and_accept();
    test_layout();
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("cluster_match_plan: ok\n");
    return 0;
}
