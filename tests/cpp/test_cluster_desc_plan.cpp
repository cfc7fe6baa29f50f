// test_cluster_desc_plan.cpp -- the host-built tables of pcc_cluster_descriptors (csrc/cluster_desc_plan.hpp) on the CPU:
//   the routing and the staging order (the SIFT batch route's clusters first, as the rounds' first table wants them),
//   the round-major to cluster-major keypoint order against a brute-force reordering,
//   the RIFT clouds' places (the concatenation, the clouds off it behind it) and
//   the output splice against a per-cluster restatement.
// usage: test_cluster_desc_plan   (exit status 0: all checks passed)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <tuple>
#include <vector>
#include "cluster_desc_plan.hpp"
#include "sift_batch_plan.hpp"

namespace {

int bad = 0;
void fail(const char* what, size_t at) {
    fprintf(stderr, "cluster desc plan: %s (at %zu)\n", what, at);
    ++bad;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t below) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33) % below;
}

void check_routes(const std::vector<size_t>& n, size_t sift_above, size_t sift_max) {
    const size_t nc = n.size();
    std::vector<size_t> off(nc + 1, 7);  // (the first offset need not be 0)
    for (size_t c = 0; c < nc; ++c) off[c + 1] = off[c] + n[c];
    const pcc::ClusterDescRoutes r = pcc::cd_routes(off.data(), nc, sift_above, sift_max);
    size_t dense = 0, sift = 0, batch = 0, total = 0;
    std::vector<unsigned char> taken;
    for (size_t c = 0; c < nc; ++c) total += n[c];
    taken.assign(total, 0);
    for (size_t c = 0; c < nc; ++c) {
        const uint32_t want = n[c] <= sift_above ? pcc::CD_DENSE : (n[c] > sift_max ? pcc::CD_SIFT_WORK : pcc::CD_SIFT_BATCH);
        if (r.route[c] != want) fail("a cluster is on the wrong route", c);
        if (r.n[c] != n[c]) fail("a cluster's size", c);
        if (r.sift_n[c] != (want == pcc::CD_SIFT_BATCH ? n[c] : 0)) fail("the rounds' size of a cluster", c);
        (want == pcc::CD_DENSE ? dense : sift) += n[c];
        if (want == pcc::CD_SIFT_BATCH) batch += n[c];
        for (size_t i = 0; i < n[c]; ++i) {
            const size_t at = (size_t)r.stage_base[c] + i;
            if (at >= total || taken[at]++) { fail("two records share a place, or one lies outside", c); break; }
        }
    }
    if (r.n_dense != dense || r.n_sift != sift || r.sift_batch_total != batch || r.stage_base[nc] != total) fail("a total", nc);
    // the staged prefix is the rounds' first concatenation
    pcc::SiftBatchRound round0;
    pcc::sift_batch_round(r.sift_n.data(), nc, 0, &round0);
    for (size_t c = 0; c < nc; ++c)
        if (r.route[c] == pcc::CD_SIFT_BATCH && round0.bases[c] != r.stage_base[c]) fail("a SIFT cluster is not where the rounds look for it", c);
    if (round0.total != batch) fail("the rounds' total", nc);
    // the others keep cluster order behind it
    size_t at = batch;
    for (size_t c = 0; c < nc; ++c) {
        if (r.route[c] == pcc::CD_SIFT_BATCH) continue;
        if (r.stage_base[c] != at) fail("a cluster off the rounds is out of order", c);
        at += n[c];
    }
}

void check_keypoint_order(size_t nc, size_t rounds) {
    std::vector<std::vector<uint32_t>> counts(rounds, std::vector<uint32_t>(nc, 0));
    std::vector<uint32_t> work(nc, 0);
    // (round, cluster) -> how many; a cluster is either in the rounds or on the work handle, or has none
    for (size_t c = 0; c < nc; ++c) {
        const uint32_t kind = rnd(4);
        if (kind == 0) continue;
        if (kind == 1) { work[c] = rnd(9); continue; }
        for (size_t r = 0; r < rounds; ++r) counts[r][c] = rnd(3) ? rnd(7) : 0;
    }
    // brute force: tag every device position with (cluster, round, i), then sort
    std::vector<std::tuple<size_t, size_t, size_t, size_t>> tagged;  // cluster, round (rounds = the work handle), i, position
    size_t pos = 0;
    for (size_t r = 0; r < rounds; ++r)
        for (size_t c = 0; c < nc; ++c)
            for (uint32_t i = 0; i < counts[r][c]; ++i) tagged.emplace_back(c, r, i, pos++);
    for (size_t c = 0; c < nc; ++c)
        for (uint32_t i = 0; i < work[c]; ++i) tagged.emplace_back(c, rounds, i, pos++);
    std::sort(tagged.begin(), tagged.end());
    std::vector<uint32_t> kbase, order;
    pcc::cd_keypoint_order(counts, work, nc, &kbase, &order);
    if (order.size() != tagged.size() || kbase.size() != nc + 1 || kbase[nc] != order.size()) { fail("the order's length", nc); return; }
    for (size_t k = 0; k < order.size(); ++k) {
        if (order[k] != std::get<3>(tagged[k])) { fail("the cluster-major order differs from the brute-force reordering", k); break; }
        const size_t c = std::get<0>(tagged[k]);
        if (!(kbase[c] <= k && k < kbase[c + 1])) { fail("a keypoint lies outside its cluster's range", k); break; }
    }
    for (size_t c = 0; c < nc; ++c)
        if (kbase[c] > kbase[c + 1]) fail("kbase decreases", c);
}

void check_clouds_and_splice(const std::vector<size_t>& q_n, size_t rift_max) {
    const size_t nc = q_n.size();
    const pcc::ClusterDescClouds p = pcc::cd_clouds(q_n.data(), nc, rift_max);
    size_t batch = 0, single = 0, total = 0;
    for (size_t c = 0; c < nc; ++c) { (q_n[c] > rift_max ? single : batch) += q_n[c]; total += q_n[c]; }
    if (p.n_batch != batch || p.n_single != single || p.bases[nc] != batch || p.dst[nc] != total) fail("a total of the clouds", nc);
    std::vector<unsigned char> taken(total, 0);
    size_t at = 0, behind = batch;
    for (size_t c = 0; c < nc; ++c) {
        const bool small = q_n[c] <= rift_max;
        if (p.small_n[c] != (small ? q_n[c] : 0)) fail("the concatenation's size of a cloud", c);
        if (p.bases[c] != at) fail("a base is not the prefix sum", c);
        if (small && p.dst[c] != at) fail("a cloud of the concatenation is not at its base", c);
        if (!small && p.dst[c] != behind) fail("a cloud off the concatenation is not behind it, in order", c);
        for (size_t i = 0; i < q_n[c]; ++i) {
            const size_t d = (size_t)p.dst[c] + i;
            if (d >= total || taken[d]++) { fail("two points share a place, or one lies outside", c); break; }
        }
        if (small) at += q_n[c]; else behind += q_n[c];
    }
    size_t queries = 0;
    for (const pcc::RiftBatchItem& it : p.items) {
        queries += it.nq;
        if ((size_t)it.base + it.n > batch) fail("an item reaches beyond the concatenation", it.base);
    }
    if (queries != batch) fail("the items do not cover the concatenation", queries);

    // the splice: the batch route keeps some rows of every small cloud, the single path some of every other
    std::vector<uint32_t> slice(nc + 1, 0);
    std::vector<size_t> single_m(nc, 0);
    for (size_t c = 0; c < nc; ++c) {
        const bool small = q_n[c] <= rift_max;
        const size_t kept = q_n[c] ? rnd((uint32_t)q_n[c] + 1) : 0;
        slice[c + 1] = slice[c] + (small ? (uint32_t)kept : 0u);
        single_m[c] = small ? 0 : kept;
    }
    std::vector<size_t> offsets;
    std::vector<pcc::ClusterDescCopy> copies;
    pcc::cd_splice(slice.data(), q_n.data(), single_m.data(), nc, rift_max, &offsets, &copies);
    // restated per cluster: where every batch row goes
    std::vector<long long> dst_of(slice[nc], -1);
    size_t out = 0;
    for (size_t c = 0; c < nc; ++c) {
        if (offsets[c] != out) fail("an output offset", c);
        if (q_n[c] <= rift_max) {
            for (uint32_t r = slice[c]; r < slice[c + 1]; ++r) dst_of[r] = (long long)out++;
        } else {
            out += single_m[c];
        }
    }
    if (offsets[nc] != out) fail("the output total", nc);
    std::vector<long long> got(slice[nc], -1);
    for (const pcc::ClusterDescCopy& cp : copies) {
        if (!cp.count) fail("an empty copy", cp.src);
        for (size_t i = 0; i < cp.count; ++i) {
            if (cp.src + i >= got.size() || got[cp.src + i] != -1) { fail("a row is copied twice, or lies outside", cp.src); break; }
            got[cp.src + i] = (long long)(cp.dst + i);
        }
    }
    if (got != dst_of) fail("the copies do not put every batch row where its cluster's slice is", nc);
    if (single == 0 && slice[nc] && (copies.size() != 1 || copies[0].src != 0 || copies[0].dst != 0 || copies[0].count != slice[nc]))
        fail("without clouds off the concatenation the splice is one copy in place", nc);
}

}  // namespace

int main() {
    const std::vector<size_t> sizes = {300, 0, 700, 701, 25, 2000, 330, 9000, 0, 8192, 8193, 1};
    for (size_t gate : {(size_t)0, (size_t)10, (size_t)700, (size_t)8192, (size_t)-1})
        for (size_t limit : {(size_t)1000, (size_t)8192, (size_t)100000}) check_routes(sizes, gate, limit);
    check_routes({}, 700, 8192);
    check_routes({0, 0}, 700, 8192);
    for (size_t nc : {(size_t)1, (size_t)3, (size_t)30})
        for (size_t rounds : {(size_t)0, (size_t)1, (size_t)5})
            for (int rep = 0; rep < 20; ++rep) check_keypoint_order(nc, rounds);
    for (size_t limit : {(size_t)50, (size_t)700, (size_t)8192}) {
        check_clouds_and_splice({300, 0, 700, 61, 0, 196, 330, 9000, 0, 51, 50}, limit);
        check_clouds_and_splice({0, 0, 0}, limit);
        check_clouds_and_splice({}, limit);
    }
    if (bad) { fprintf(stderr, "cluster desc plan: %d checks FAILED\n", bad); return 1; }
    printf("cluster desc plan: routes, keypoint order, clouds and splice ok\n");
    return 0;
}
