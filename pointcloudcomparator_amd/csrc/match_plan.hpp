// match_plan.hpp -- the host plan the descriptor searches share (match_batch.hip, match_dims.hip through match_dims_plan.hpp,
// cluster_match.hip through cluster_match_plan.hpp): the work item, the slice rule, the table of work items and the
// de-duplication of the reference clouds.  Plain C++ (no HIP): tests/cpp/test_match_plan.cpp compiles it on its own.
//
// One work item = 64 consecutive queries of ONE pair against one slice of that pair's references; every query of a pair is in
// exactly one item per slice of its references and no item crosses a pair.  Slices keep the workgroups of a 23 528-reference pair
// from running fifty times longer than those of a 400-reference pair; the slices of a query block merge in device memory.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <unordered_map>
#include <utility>
#include <vector>

namespace pcc {

constexpr unsigned int MATCH_SLICE_MIN = 256;  // references per work item at least (16 per wave of a 16-wave workgroup) ...
constexpr size_t MATCH_ITEMS_WANTED = 1024;    // ... when the table would otherwise leave most of the chip idle: two workgroups of
                                               // 1024 lanes per CU, 256 CUs, twice over
constexpr size_t MATCH_LIMIT = 1ull << 31;     // records, result slots and items of one call stay below it

// References per work item at most, for records of dp floats (4, 8, 16, 32).  An item's time grows with 3 * dim + 3 operations a
// pair where the 3-D search has 12, so beyond dp = 8 the slice shrinks in proportion: the longest item then stays within 2.5
// times the 3-D kernel's longest (99 x 512 against 12 x 2048 + the merge) while the table has at most four times as many items.
inline unsigned int match_dims_slice_max(int dp) { return dp <= 8 ? 2048u : dp == 16 ? 1024u : 512u; }
// the 3-D search's records are four floats (x, y, z and a validity word)
inline unsigned int match_slice_max_3d() { return match_dims_slice_max(4); }

// one workgroup's work: queries rec[q0 .. q0 + nq) against references rec[r0 .. r0 + nr), in records; the references' indices in
// their own cloud are ridx0 ...; results for query q0 + i go to slot qslot0 + i
struct MatchItem {
    uint32_t q0, nq, r0, nr, ridx0, qslot0, pad0, pad1;
};

// a pair to search, in records and result slots; nq == 0 or nr == 0: nothing to search, no item
struct MatchPair {
    size_t q_rec0, nq, r_rec0, nr, slot0;
};

inline size_t match_items_at(const std::vector<MatchPair>& pairs, unsigned int slice) {
    size_t c = 0;
    for (const MatchPair& p : pairs)
        if (p.nq && p.nr) c += ((p.nq + 63) / 64) * ((p.nr + slice - 1) / slice);
    return c;
}

// the slice rule: from slice_max, halved down to MATCH_SLICE_MIN while fewer than MATCH_ITEMS_WANTED items result
inline unsigned int match_slice(const std::vector<MatchPair>& pairs, unsigned int slice_max) {
    unsigned int slice = slice_max;
    while (slice > MATCH_SLICE_MIN && match_items_at(pairs, slice) < MATCH_ITEMS_WANTED) slice /= 2;
    return slice;
}

// The table: the widest pairs first (their many slices start while the short items fill the gaps behind them; pairs of equal
// width in the order given), query blocks the outer loop, slices the inner.  false: MATCH_LIMIT items and more (none is built).
inline bool match_items(const std::vector<MatchPair>& pairs, unsigned int slice, std::vector<MatchItem>* items) {
    items->clear();
    const size_t n_items = match_items_at(pairs, slice);
    if (n_items >= MATCH_LIMIT) return false;
    items->reserve(n_items);
    std::vector<size_t> order(pairs.size());
    for (size_t p = 0; p < pairs.size(); ++p) order[p] = p;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return pairs[a].nr > pairs[b].nr; });
    for (size_t p : order) {
        const MatchPair& pr = pairs[p];
        if (!pr.nq || !pr.nr) continue;
        for (size_t qb = 0; qb < pr.nq; qb += 64)
            for (size_t rb = 0; rb < pr.nr; rb += slice) {
                MatchItem it;
                it.q0 = (uint32_t)(pr.q_rec0 + qb);
                it.nq = (uint32_t)std::min<size_t>(64, pr.nq - qb);
                it.r0 = (uint32_t)(pr.r_rec0 + rb);
                it.nr = (uint32_t)std::min<size_t>(slice, pr.nr - rb);
                it.ridx0 = (uint32_t)rb;
                it.qslot0 = (uint32_t)(pr.slot0 + qb);
                it.pad0 = it.pad1 = 0;
                items->push_back(it);
            }
    }
    return true;
}

// ---- the plan of a call that names its clouds by pointer (pcc_match_knn_batch, pcc_match_knn_batch_dims) -------------------------
struct MatchPlan {
    struct Cloud { const void* p; size_t n, rec0; };
    std::vector<Cloud> clouds;      // every DISTINCT (pointer, length) of des1 once, in order of first appearance
    std::vector<size_t> cloud_of;   // per pair: its reference cloud
    std::vector<size_t> q_rec0;     // per pair: first record of its queries
    std::vector<size_t> q_slot0;    // n_pairs + 1: first result slot of its queries; [n_pairs] = all slots
    size_t n_rec = 0, n_slots = 0;  // records (references of distinct clouds, then queries); result slots (= queries)
    unsigned int slice = 0;         // references per item at most
    std::vector<MatchItem> items;
};

struct PtrLenHash {
    size_t operator()(const std::pair<const void*, size_t>& k) const {
        return std::hash<const void*>()(k.first) ^ (std::hash<size_t>()(k.second) * 0x9e3779b97f4a7c15ull);
    }
};

// Lays the records out (a reference cloud that several pairs name is laid out once) and builds the table.
// false: MATCH_LIMIT records or items and more (nothing usable in *plan).
inline bool match_plan(size_t n_pairs, const void* const* des1, const size_t* n1, const size_t* n2, unsigned int slice_max, MatchPlan* plan) {
    MatchPlan& pl = *plan;
    pl.clouds.clear();
    pl.items.clear();
    pl.cloud_of.assign(n_pairs, 0);
    pl.q_rec0.assign(n_pairs, 0);
    pl.q_slot0.assign(n_pairs + 1, 0);
    pl.n_rec = pl.n_slots = 0;
    std::unordered_map<std::pair<const void*, size_t>, size_t, PtrLenHash> seen;
    for (size_t p = 0; p < n_pairs; ++p) {
        const auto key = std::make_pair(des1[p], n1[p]);
        auto f = seen.find(key);
        if (f == seen.end()) {
            f = seen.emplace(key, pl.clouds.size()).first;
            pl.clouds.push_back({des1[p], n1[p], pl.n_rec});
            pl.n_rec += n1[p];
        }
        pl.cloud_of[p] = f->second;
    }
    std::vector<MatchPair> pairs(n_pairs);
    for (size_t p = 0; p < n_pairs; ++p) {
        pl.q_rec0[p] = pl.n_rec;
        pl.q_slot0[p] = pl.n_slots;
        pairs[p] = {pl.n_rec, n2[p], pl.clouds[pl.cloud_of[p]].rec0, n1[p], pl.n_slots};
        pl.n_rec += n2[p];
        pl.n_slots += n2[p];
    }
    pl.q_slot0[n_pairs] = pl.n_slots;
    if (pl.n_rec >= MATCH_LIMIT) return false;
    pl.slice = match_slice(pairs, slice_max);
    return match_items(pairs, pl.slice, &pl.items);
}

}  // namespace pcc
