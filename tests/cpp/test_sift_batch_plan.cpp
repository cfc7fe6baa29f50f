// test_sift_batch_plan.cpp -- the host-built tables of pcc_sift_keypoints_batch (csrc/sift_batch_plan.hpp) on the CPU: for the
// table in front of the first round and for every round after it, every (cloud, point) is a query of exactly one item, no item
// crosses a cloud, empty clouds and clouds that fell below the gate have no items and no points, the bases are the prefix
// sums -- also behind a round in which some clouds shrank to zero -- and the splice of the rounds' keypoints is a permutation.
// usage: test_sift_batch_plan [n0 n1 ...]   (the sizes of the first round; default: tests/test_sift_batch_cpu.py's)
//   The later rounds are made up here: cloud c keeps (n * (3 + c % 3)) / 8 of its points per round until every cloud is gone.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "sift_batch_plan.hpp"

namespace {

int bad = 0;
void fail(const char* what, size_t round, size_t at) {
    fprintf(stderr, "sift batch plan: %s (round %zu, at %zu)\n", what, round, at);
    ++bad;
}

// one round's table against the sizes it was built from
void check_round(const pcc::SiftBatchRound& r, const std::vector<size_t>& sizes, size_t min_points, size_t round) {
    const size_t nc = sizes.size();
    if (r.n.size() != nc || r.bases.size() != nc + 1 || r.bases64.size() != nc + 1) { fail("a table has the wrong length", round, nc); return; }
    size_t total = 0;
    for (size_t c = 0; c < nc; ++c) {
        const size_t want = sizes[c] >= min_points ? sizes[c] : 0;
        if (r.n[c] != want) fail(want ? "a cloud above the gate lost its points" : "a dropped cloud kept points", round, c);
        if (r.bases[c] != total || r.bases64[c] != (int64_t)total) fail("a base is not the prefix sum", round, c);
        total += want;
    }
    if (r.bases[nc] != total || r.bases64[nc] != (int64_t)total || r.total != total) fail("the last base is not the total", round, nc);
    if (bad) return;
    std::vector<unsigned int> covered(total, 0u);
    for (size_t k = 0; k < r.items.size() && bad == 0; ++k) {
        const pcc::RiftBatchItem& it = r.items[k];
        size_t c = 0;
        while (c < nc && !(r.bases[c] == it.base && r.n[c] == it.n && r.n[c] > 0)) ++c;
        if (c == nc) { fail("an item names an empty or dropped cloud, or none", round, k); break; }
        if (it.nq == 0 || it.nq > pcc::RB_QUERIES) fail("an item with no query, or more than a block", round, k);
        if ((size_t)it.q0 + it.nq > it.n) fail("an item's queries cross the end of its cloud", round, k);
        for (uint32_t q = 0; q < it.nq && bad == 0; ++q) ++covered[(size_t)it.base + it.q0 + q];
    }
    for (size_t i = 0; i < total && bad == 0; ++i)
        if (covered[i] != 1) fail("a point is not the query of exactly one item", round, i);
}

}  // namespace

int main(int argc, char** argv) {
    std::vector<size_t> n = {300, 0, 24, 25, 600, 2049, 0, 8000, 26};
    if (argc > 1) {
        n.clear();
        for (int i = 1; i < argc; ++i) n.push_back((size_t)strtoull(argv[i], nullptr, 10));
    }
    const size_t nc = n.size(), gate = 25;
    pcc::SiftBatchRound r;
    pcc::sift_batch_round(n.data(), nc, 0, &r);  // the caller's clouds: no gate
    check_round(r, n, 0, 0);
    std::vector<std::vector<uint32_t>> counts;
    std::vector<uint32_t> sizes(n.begin(), n.end());
    size_t rounds = 0, dropped_with_points = 0;
    while (bad == 0 && r.total > 0 && rounds < 64) {
        // what a voxel stage would report: every cloud still in the batch shrinks, some to below the gate, some to zero
        for (size_t c = 0; c < nc; ++c) sizes[c] = (uint32_t)(r.n[c] * (3 + c % 3) / 8);
        if (rounds == 1 && nc > 0) sizes[0] = 0;  // a cloud that shrinks to nothing in the middle of the batch
        std::vector<size_t> as_size(sizes.begin(), sizes.end());
        for (size_t c = 0; c < nc; ++c) dropped_with_points += sizes[c] > 0 && sizes[c] < gate;
        pcc::sift_batch_round(sizes.data(), nc, gate, &r);
        ++rounds;
        check_round(r, as_size, gate, rounds);
        std::vector<uint32_t> found(nc);
        for (size_t c = 0; c < nc; ++c) found[c] = (uint32_t)((r.n[c] + c + rounds) % 7);  // keypoints of the round, some clouds none
        counts.push_back(found);
    }
    if (r.total != 0) fail("the batch never emptied", rounds, r.total);
    // the splice: round-major rows -> (cloud, round) order, every row exactly once, offsets = the per-cloud sums
    std::vector<size_t> offsets;
    std::vector<pcc::SiftBatchCopy> copies;
    pcc::sift_batch_splice(counts, nc, &offsets, &copies);
    size_t total = 0;
    for (size_t c = 0; c < nc && bad == 0; ++c) {
        if (offsets[c] != total) fail("a slice bound is not the sum of the clouds before", 0, c);
        for (const std::vector<uint32_t>& f : counts) total += f[c];
    }
    if (bad == 0 && (offsets.size() != nc + 1 || offsets[nc] != total)) fail("the last slice bound is not the total", 0, nc);
    std::vector<unsigned int> read(total, 0u), written(total, 0u);
    std::vector<size_t> round_cloud_src;  // where (round, cloud) starts in the round-major buffer
    size_t dst_before = 0;
    for (const pcc::SiftBatchCopy& cp : copies) {
        if (bad) break;
        if (cp.count == 0 || cp.src + cp.count > total || cp.dst + cp.count > total) { fail("a copy is empty or leaves the arrays", 0, cp.dst); break; }
        if (cp.dst != dst_before) fail("the copies do not fill the result front to back", 0, cp.dst);
        dst_before = cp.dst + cp.count;
        for (size_t i = 0; i < cp.count; ++i) { ++read[cp.src + i]; ++written[cp.dst + i]; }
    }
    for (size_t i = 0; i < total && bad == 0; ++i)
        if (read[i] != 1 || written[i] != 1) fail("a keypoint is not copied exactly once", 0, i);
    // the source of every (cloud, round) is where the rounds before and the clouds before it in its round end
    {
        size_t k = 0, round_at = 0;
        std::vector<std::vector<size_t>> src(counts.size(), std::vector<size_t>(nc, 0));
        for (size_t q = 0; q < counts.size(); ++q)
            for (size_t c = 0; c < nc; ++c) { src[q][c] = round_at; round_at += counts[q][c]; }
        for (size_t c = 0; c < nc && bad == 0; ++c)
            for (size_t q = 0; q < counts.size() && bad == 0; ++q) {
                if (!counts[q][c]) continue;
                if (k >= copies.size() || copies[k].src != src[q][c] || copies[k].count != counts[q][c]) fail("a copy does not name its round's rows", q, c);
                ++k;
            }
        if (bad == 0 && k != copies.size()) fail("more copies than (cloud, round) pairs with keypoints", 0, k);
    }
    if (bad) return 1;
    size_t points = 0;
    for (size_t v : n) points += v;
    printf("sift batch plan ok: %zu clouds, %zu points, %zu rounds, %zu clouds dropped below the gate with points left, %zu keypoints spliced, tile %u\n",
           nc, points, rounds, dropped_with_points, total, pcc::RB_TILE);
    return 0;
}
