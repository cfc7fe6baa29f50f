// test_vfh_batch_plan.cpp -- the host side of pcc_vfh_descriptors_batch (csrc/vfh_batch_plan.hpp) on the CPU: the routes at
// sizes limit - 1 / limit / limit + 1 and 0 / 1 / 2, clusters on alternating routes, the caller's bounds as prefix sums of
// (n >= 2), the bases and row-builder items of the batch route, the vote items (every batch-route point in exactly one item, no
// item across a cluster), the copy runs of a host caller (every staged row exactly once, in cluster order), limit 0, and the
// refusals of the offsets (a decrease, 2^31 points).
// usage: test_vfh_batch_plan   (no arguments; exit status 0 and one line "vfh batch plan ok: ..." when every case holds)
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "vfh_batch_plan.hpp"

namespace {

int g_bad = 0;
void fail(const char* what, size_t at) { fprintf(stderr, "vfh batch plan: %s (at %zu)\n", what, at); ++g_bad; }

std::vector<size_t> offsets_of(const std::vector<size_t>& sizes, size_t first) {
    std::vector<size_t> off(sizes.size() + 1, first);
    for (size_t c = 0; c < sizes.size(); ++c) off[c + 1] = off[c] + sizes[c];
    return off;
}

// every property of one plan; returns the number of copy runs
size_t check_case(const std::vector<size_t>& sizes, size_t limit, size_t first) {
    const size_t nc = sizes.size();
    const std::vector<size_t> off = offsets_of(sizes, first);
    if (pcc::check_range_offsets(off.data(), nc) != pcc::RANGE_OFFSETS_OK) fail("good offsets are refused", nc);
    const pcc::VfhBatchPlan p = pcc::vfh_batch_plan(off.data(), nc, limit);
    if (p.n.size() != nc || p.small_n.size() != nc || p.src.size() != nc + 1 || p.bases.size() != nc + 1 || p.row.size() != nc ||
        p.out_offsets.size() != nc + 1) {
        fail("a table has the wrong length", nc);
        return 0;
    }
    // routes, bases, bounds
    size_t at = 0, rows = 0, n_brute = 0, n_large = 0, n_route = 0;
    for (size_t c = 0; c < nc; ++c) {
        const size_t n = sizes[c];
        if (p.n[c] != n) fail("a cluster's size is wrong", c);
        if (p.src[c] != off[c] - first) fail("a cluster's place among the records is wrong", c);
        const bool none = n < 2, large = !none && n > limit, batch = !none && !large;
        if (p.on_work_handle(c) != large || p.on_batch_route(c) != batch) fail("a cluster is on the wrong route", c);
        if (p.small_n[c] != (batch ? n : 0)) fail("a cluster's size on the batch route is wrong", c);
        if (p.bases[c] != at) fail("a base is not the prefix sum of the batch route's sizes", c);
        if (p.out_offsets[c] != rows || p.row[c] != rows) fail("an output bound is not the prefix sum of (n >= 2)", c);
        if (batch) {
            if (n_route >= p.route.size() || p.route[n_route] != c) fail("the route list misses a cluster or is out of order", c);
            ++n_route;
            n_brute += n;
            at += n;
        }
        if (large) n_large += n;
        rows += none ? 0 : 1;
    }
    if (n_route != p.route.size()) fail("the route list names a cluster off the batch route", n_route);
    if (p.bases[nc] != at || p.src[nc] != off[nc] - first || p.out_offsets[nc] != rows || p.descriptors() != rows) fail("the last entries are not the totals", nc);
    if (p.n_brute != n_brute || p.n_large != n_large || n_brute != at) fail("the points per route are wrong", nc);
    // the row builder's items: every point of the batch route a query of exactly one item, no item crosses a cluster
    std::vector<unsigned int> covered(at, 0u);
    for (size_t k = 0; k < p.items.size(); ++k) {
        const pcc::RiftBatchItem& it = p.items[k];
        size_t c = 0;
        while (c < nc && !(p.bases[c] == it.base && p.small_n[c] == it.n && it.n > 0)) ++c;
        if (c == nc) { fail("an item names no cluster of the batch route", k); continue; }
        if (it.nq == 0 || it.nq > pcc::RB_QUERIES || (size_t)it.q0 + it.nq > it.n) { fail("an item's queries are out of its cluster", k); continue; }
        for (uint32_t q = 0; q < it.nq; ++q) ++covered[(size_t)it.base + it.q0 + q];
    }
    for (size_t i = 0; i < at; ++i)
        if (covered[i] != 1) { fail("a point of the batch route is not a query exactly once", i); break; }
    // the vote items: every point of the batch route in exactly one item, no item crosses a cluster, in cluster order
    std::vector<unsigned int> voted(at, 0u);
    size_t last_first = 0;
    for (size_t k = 0; k < p.votes.size(); ++k) {
        const pcc::VfhVoteItem& v = p.votes[k];
        if (v.cluster >= nc || !p.on_batch_route(v.cluster)) { fail("a vote item names no cluster of the batch route", k); continue; }
        if (v.count == 0 || v.count > pcc::VFH_BATCH_VOTE_POINTS) { fail("a vote item is empty or too large", k); continue; }
        if (v.first < p.bases[v.cluster] || (size_t)v.first + v.count > (size_t)p.bases[v.cluster] + p.small_n[v.cluster]) {
            fail("a vote item crosses its cluster", k);
            continue;
        }
        if (k && v.first < last_first) fail("the vote items are not in order", k);
        last_first = v.first;
        for (uint32_t i = 0; i < v.count; ++i) ++voted[(size_t)v.first + i];
    }
    for (size_t i = 0; i < at; ++i)
        if (voted[i] != 1) { fail("a point of the batch route is not in exactly one vote item", i); break; }
    // the copy runs: every row of a batch-route cluster exactly once, no row of the work handle, in cluster order, merged
    std::vector<unsigned int> copied(rows, 0u);
    size_t last_end = 0;
    for (size_t k = 0; k < p.copies.size(); ++k) {
        const pcc::VfhBatchCopy& cp = p.copies[k];
        if (cp.count == 0 || cp.row + cp.count > rows) { fail("a copy is empty or out of range", k); continue; }
        if (k && cp.row < last_end) fail("the copies are not in cluster order", k);
        if (k && cp.row == last_end) fail("two neighbouring copies were not merged", k);
        last_end = cp.row + cp.count;
        for (size_t i = 0; i < cp.count; ++i) ++copied[cp.row + i];
    }
    for (size_t c = 0; c < nc; ++c) {
        if (sizes[c] < 2) continue;
        const unsigned int want = p.on_batch_route(c) ? 1u : 0u;  // (the work handle writes its row itself)
        if (copied[p.out_offsets[c]] != want) fail(want ? "a staged row is not copied exactly once" : "a row of the work handle is copied", c);
    }
    return p.copies.size();
}

}  // namespace

int main() {
    size_t cases = 0;
    const size_t V = pcc::VFH_BATCH_VOTE_POINTS;
    // sizes limit - 1, limit, limit + 1, for a small limit and the default: the runs between the clusters on the work handle
    for (size_t limit : {(size_t)500, (size_t)8192}) {
        const size_t copies = check_case({limit - 1, limit, limit + 1, 0, 3, limit + 1, limit}, limit, 11);
        if (copies != 3) fail("the copy list is not merged into the runs between the large clusters", copies);  // {l - 1, l}, {3}, {l}
        ++cases;
    }
    // sizes 0, 1, 2: no row, no row, one row; small clusters in front, in the middle and at the end do not break a run
    if (check_case({0, 1, 2}, 8192, 0) != 1) fail("sizes 0, 1, 2 do not give one run of one row", 0);
    if (check_case({1, 0, 5, 0, 1, 64, 65, 1, 0}, 8192, 3) != 1) fail("clusters without a row split the run", 0);
    check_case({0}, 8192, 7);
    check_case({1}, 8192, 7);
    check_case({}, 8192, 3);
    cases += 5;
    // clusters on alternating routes: every batch-route row is a run of its own
    if (check_case({20, 600, 30, 700, 1, 40, 800, 2}, 500, 5) != 4) fail("alternating routes do not give one run per batch-route cluster", 0);
    ++cases;
    // the vote items around their size
    check_case({V - 1, V, V + 1, 2 * V, 2 * V + 1, 3}, 8192, 0);
    ++cases;
    // limit 0 puts every cluster of 2 points and more on the work handle: no batch route, no copies
    if (check_case({4, 0, 9, 1, 2}, 0, 0) != 0) fail("copies without a batch route", 0);
    // limit 1: the same (a cluster of 1 point is on neither route)
    if (check_case({4, 1, 2}, 1, 0) != 0) fail("copies without a batch route", 1);
    // every cluster on the batch route and contiguous: one copy
    if (check_case({300, 600, 700}, 8192, 100) != 1) fail("a contiguous batch is not one copy", 0);
    cases += 3;

    // the 2^31 refusals of the offsets
    {
        const size_t dec[] = {0, 5, 4, 9};
        size_t bad = 99;
        if (pcc::check_range_offsets(dec, 3, &bad) != pcc::RANGE_OFFSETS_DECREASE || bad != 1) fail("a decrease is not refused at its cluster", bad);
        const size_t big = (size_t)1 << 31;
        const size_t at_limit[] = {10, 10 + big - 1}, over[] = {10, 10 + big}, both[] = {0, big, big - 1};
        if (pcc::check_range_offsets(at_limit, 1) != pcc::RANGE_OFFSETS_OK) fail("2^31 - 1 points are refused", 0);
        if (pcc::check_range_offsets(over, 1) != pcc::RANGE_OFFSETS_TOO_MANY) fail("2^31 points are not refused", 0);
        if (pcc::check_range_offsets(both, 2) != pcc::RANGE_OFFSETS_DECREASE) fail("a decrease does not come before the size", 0);
        if (pcc::check_range_offsets(dec, (size_t)1 << 31) != pcc::RANGE_OFFSETS_DECREASE) fail("a decrease does not come before 2^31 clusters", 0);
        cases += 5;
    }
    if (g_bad) return 1;
    printf("vfh batch plan ok: %zu cases\n", cases);
    return 0;
}
