// test_fpfh_batch_plan.cpp -- the host side of pcc_fpfh_descriptors_batch (csrc/range_batch_plan.hpp, csrc/fpfh_batch_plan.hpp) on the CPU: the routes at
// sizes limit - 1 / limit / limit + 1, empty clusters that share a base, the bases and work items of the batch route, the copy
// list tiling the output exactly once in cluster order, and the refusals of the offsets (a decrease, 2^31 points).
// usage: test_fpfh_batch_plan   (no arguments; exit status 0 and one line "fpfh batch plan ok: ..." when every case holds)
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "fpfh_batch_plan.hpp"

namespace {

int g_bad = 0;
void fail(const char* what, size_t at) { fprintf(stderr, "fpfh batch plan: %s (at %zu)\n", what, at); ++g_bad; }

std::vector<size_t> offsets_of(const std::vector<size_t>& sizes, size_t first) {
    std::vector<size_t> off(sizes.size() + 1, first);
    for (size_t c = 0; c < sizes.size(); ++c) off[c + 1] = off[c] + sizes[c];
    return off;
}

// every property of one plan; kept[c]: the rows cluster c ends with (whichever route), <= its size
size_t check_case(const std::vector<size_t>& sizes, size_t limit, size_t first, const std::vector<size_t>& kept) {
    const size_t nc = sizes.size();
    const std::vector<size_t> off = offsets_of(sizes, first);
    if (pcc::check_range_offsets(off.data(), nc) != pcc::RANGE_OFFSETS_OK) fail("good offsets are refused", nc);
    const pcc::RangeBatchPlan p = pcc::range_batch_plan(off.data(), nc, 0, limit);
    if (p.n.size() != nc || p.small_n.size() != nc || p.src.size() != nc + 1 || p.bases.size() != nc + 1) { fail("a table has the wrong length", nc); return 0; }
    size_t at = 0, n_brute = 0, n_large = 0;
    for (size_t c = 0; c < nc; ++c) {
        if (p.n[c] != sizes[c]) fail("a cluster's size is wrong", c);
        if (p.src[c] != off[c] - first) fail("a cluster's place among the records is wrong", c);
        const bool large = sizes[c] > limit;
        if (p.on_work_handle(c) != large) fail("a cluster is on the wrong route", c);
        if (p.small_n[c] != (large ? 0 : sizes[c])) fail("a cluster's size on the batch route is wrong", c);
        if (p.bases[c] != at) fail("a base is not the prefix sum of the batch route's sizes", c);
        (large ? n_large : n_brute) += sizes[c];
        at += large ? 0 : sizes[c];
    }
    if (p.bases[nc] != at || p.src[nc] != off[nc] - first) fail("the last entries are not the totals", nc);
    if (p.n_brute != n_brute || p.n_large != n_large || n_brute != at) fail("the points per route are wrong", nc);
    // the work items: every point of the batch route a query of exactly one item, no item crosses a cluster
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
    // the splice: slice bounds as the finish kernel leaves them, the work handle's counts
    std::vector<unsigned int> slice(nc + 1, 0u);
    std::vector<size_t> single_m(nc, 0);
    for (size_t c = 0; c < nc; ++c) {
        slice[c + 1] = slice[c] + (unsigned int)(p.on_work_handle(c) ? 0 : kept[c]);
        if (p.on_work_handle(c)) single_m[c] = kept[c];
    }
    std::vector<size_t> out_off;
    std::vector<pcc::FpfhBatchCopy> copies;
    pcc::fpfh_batch_splice(p, slice.data(), single_m.data(), &out_off, &copies);
    if (out_off.size() != nc + 1) { fail("the output bounds have the wrong length", nc); return 0; }
    size_t rows = 0;
    for (size_t c = 0; c < nc; ++c) {
        if (out_off[c] != rows) fail("an output bound is not the prefix sum of the kept rows", c);
        rows += kept[c];
    }
    if (out_off[nc] != rows) fail("the last output bound is not the total", nc);
    // the copies tile the batch route's rows and their places in the output exactly once, in cluster order
    std::vector<int> owner(rows, -1);        // output row -> the batch row copied there
    std::vector<unsigned int> used(slice[nc], 0u);
    size_t last_src = 0, last_dst = 0;
    for (size_t k = 0; k < copies.size(); ++k) {
        const pcc::FpfhBatchCopy& cp = copies[k];
        if (cp.count == 0 || cp.src + cp.count > slice[nc] || cp.dst + cp.count > rows) { fail("a copy is empty or out of range", k); continue; }
        if (k && (cp.src < last_src || cp.dst < last_dst)) fail("the copies are not in cluster order", k);
        if (k && cp.src == last_src && cp.dst == last_dst) fail("two neighbouring copies were not merged", k);
        last_src = cp.src + cp.count;
        last_dst = cp.dst + cp.count;
        for (size_t i = 0; i < cp.count; ++i) {
            if (owner[cp.dst + i] != -1) fail("an output row is written twice", cp.dst + i);
            owner[cp.dst + i] = (int)(cp.src + i);
            ++used[cp.src + i];
        }
    }
    for (size_t i = 0; i < used.size(); ++i)
        if (used[i] != 1) { fail("a row of the batch route is not copied exactly once", i); break; }
    for (size_t c = 0; c < nc; ++c)
        for (size_t i = 0; i < kept[c]; ++i) {
            const int want = p.on_work_handle(c) ? -1 : (int)(slice[c] + i);  // (the work handle writes its rows itself)
            if (owner[out_off[c] + i] != want) { fail("an output row holds the wrong row", out_off[c] + i); break; }
        }
    return copies.size();
}

}  // namespace

int main() {
    size_t cases = 0;
    // routes around the limit, for a small limit and the default
    for (size_t limit : {(size_t)500, (size_t)8192}) {
        const std::vector<size_t> sizes = {limit - 1, limit, limit + 1, 0, 3, limit + 1, limit};
        std::vector<size_t> kept(sizes);
        for (size_t& k : kept) k -= k / 7;
        const size_t copies = check_case(sizes, limit, 11, kept);
        // (the runs between the clusters on the work handle: {limit - 1, limit}, {3}, {limit})
        if (copies != 3) fail("the copy list is not merged into the runs between the large clusters", copies);
        ++cases;
    }
    // empty clusters that share a base, in front, in the middle and at the end; nothing kept of some clusters
    check_case({0, 0, 5, 0, 0, 64, 65, 0}, 8192, 0, {0, 0, 5, 0, 0, 0, 65, 0});
    check_case({0}, 8192, 7, {0});
    check_case({}, 8192, 3, {});
    // every cluster on the work handle: no batch route at all (limit 0 sends every non-empty cluster there)
    if (check_case({4, 0, 9}, 0, 0, {4, 0, 2}) != 0) fail("copies without a batch route", 0);
    // every cluster on the batch route and contiguous: one copy
    if (check_case({300, 600, 700}, 8192, 100, {300, 600, 700}) != 1) fail("a contiguous batch is not one copy", 0);
    // a gap in the kept rows of the batch route does not break the run: the rows stay neighbours on both sides
    if (check_case({300, 600, 700}, 8192, 0, {300, 0, 700}) != 1) fail("an empty slice split the run", 0);
    cases += 6;

    // the offsets' refusals
    {
        const size_t dec[] = {0, 5, 4, 9};
        size_t bad = 99;
        if (pcc::check_range_offsets(dec, 3, &bad) != pcc::RANGE_OFFSETS_DECREASE || bad != 1) fail("a decrease is not refused at its cluster", bad);
        const size_t big = (size_t)1 << 31;
        const size_t at_limit[] = {10, 10 + big - 1}, over[] = {10, 10 + big}, both[] = {0, big, big - 1};
        if (pcc::check_range_offsets(at_limit, 1) != pcc::RANGE_OFFSETS_OK) fail("2^31 - 1 points are refused", 0);
        if (pcc::check_range_offsets(over, 1) != pcc::RANGE_OFFSETS_TOO_MANY) fail("2^31 points are not refused", 0);
        if (pcc::check_range_offsets(both, 2) != pcc::RANGE_OFFSETS_DECREASE) fail("a decrease does not come before the size", 0);
        if (pcc::check_range_offsets(dec, 0) != pcc::RANGE_OFFSETS_OK) fail("no cluster: nothing to refuse", 0);
        cases += 5;
    }
    if (g_bad) return 1;
    printf("fpfh batch plan ok: %zu cases\n", cases);
    return 0;
}
