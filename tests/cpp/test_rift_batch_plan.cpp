// test_rift_batch_plan.cpp -- the host-built work-item table of pcc_rift_descriptors_batch (csrc/rift_batch_plan.hpp) on the
// CPU: every (cloud, query) is covered exactly once, no item crosses a cloud, the bases are the prefix sums.
// usage: test_rift_batch_plan [n0 n1 ...]   (default: the sizes tests/test_rift_batch_cpu.py names)
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "rift_batch_plan.hpp"

int main(int argc, char** argv) {
    std::vector<size_t> n = {0, 1, 64, 65, 2048, 2049, 0, 700};
    if (argc > 1) {
        n.clear();
        for (int i = 1; i < argc; ++i) n.push_back((size_t)strtoull(argv[i], nullptr, 10));
    }
    std::vector<uint32_t> bases;
    std::vector<pcc::RiftBatchItem> items;
    const unsigned int block = pcc::rift_batch_plan(n.data(), n.size(), &bases, &items);
    int bad = 0;
    auto fail = [&](const char* what, size_t at) { fprintf(stderr, "rift batch plan: %s (at %zu)\n", what, at); ++bad; };
    if (block < pcc::RB_QUERIES_MIN || block > pcc::RB_QUERIES || (block & (block - 1))) fail("the query block is not one of 4 ... 64", block);
    if (bases.size() != n.size() + 1) fail("bases has the wrong length", bases.size());
    size_t total = 0;
    for (size_t c = 0; c < n.size() && bad == 0; ++c) {
        if (bases[c] != total) fail("a base is not the prefix sum", c);
        total += n[c];
    }
    if (bad == 0 && bases[n.size()] != total) fail("the last base is not the total", n.size());
    std::vector<unsigned int> covered(total, 0u);
    for (size_t k = 0; k < items.size() && bad == 0; ++k) {
        const pcc::RiftBatchItem& it = items[k];
        // the item's cloud is one of the batch's, whole
        size_t c = 0;
        while (c < n.size() && !(bases[c] == it.base && n[c] == it.n && n[c] > 0)) ++c;
        if (c == n.size()) { fail("an item names no cloud of the batch", k); break; }
        if (it.nq == 0 || it.nq > block) fail("an item with no query, or more than a block", k);
        if ((size_t)it.q0 + it.nq > it.n) fail("an item's queries cross the end of its cloud", k);
        if (it.q0 % block) fail("a query block does not start on a block boundary", k);
        for (uint32_t q = 0; q < it.nq && bad == 0; ++q) ++covered[(size_t)it.base + it.q0 + q];
    }
    for (size_t i = 0; i < total && bad == 0; ++i)
        if (covered[i] != 1) fail("a query is not covered exactly once", i);
    size_t want_items = 0;
    for (size_t v : n) want_items += (v + block - 1) / block;
    if (items.size() != want_items) fail("the table has the wrong number of items", items.size());
    // the block is the largest that fills the table, or the smallest there is
    if (block > pcc::RB_QUERIES_MIN && items.size() < pcc::RB_ITEMS_WANTED) fail("a larger block than the table can afford", block);
    if (block < pcc::RB_QUERIES) {
        size_t coarser = 0;
        for (size_t v : n) coarser += (v + 2 * block - 1) / (2 * block);
        if (coarser >= pcc::RB_ITEMS_WANTED) fail("a smaller block than the table needs", block);
    }
    if (bad) return 1;
    printf("rift batch plan ok: %zu clouds, %zu points, %zu items of up to %u queries, tile %u\n", n.size(), total, items.size(),
           block, pcc::RB_TILE);
    return 0;
}
