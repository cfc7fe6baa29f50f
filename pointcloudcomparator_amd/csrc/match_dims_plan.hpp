// match_dims_plan.hpp -- the host side of pcc_match_knn_batch_dims for dim != 3 (match_dims.hip): the packed record, the
// de-duplication of the reference clouds and the table of work items.  Plain C++ (no HIP): tests/cpp/test_match_dims_plan.cpp
// compiles it on its own.
//
// The record: DP floats, DP = the smallest of 4, 8, 16, 32 that holds `dim`; floats dim .. DP-1 are +0.  A padded term of the
// distance is (0 - 0) * (0 - 0) = +0 and d + 0 == d for every d >= 0 and for +inf, so the padded sum has the bits of the sum
// over `dim` terms.  A record whose first `dim` floats are not all finite (PCL's isValid over nr_dimensions) is packed as
// (+inf, 0, ... 0): its distance to every valid record is +inf and to another invalid one NaN, both "no neighbour" by
// key_none -- the kernel needs no test on the record, and neither side of such a pair is ever reported.
//
// The table: as match_batch.hip's.  One work item = 64 consecutive queries of ONE pair against one slice of that pair's
// references; every query of a pair is in exactly one item per slice of its references and no item crosses a pair.  An item's
// time grows with 3 * dim + 3 operations a pair where the 3-D search has 12, so beyond DP = 8 the slice shrinks in proportion
// (2048 references at DP <= 8, 1024 at 16, 512 at 32): the longest item then stays within 2.5 times the 3-D kernel's longest
// (99 x 512 against 12 x 2048 + the merge) while the table has at most four times as many items.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <limits>
#include <unordered_map>
#include <utility>
#include <vector>

namespace pcc {

constexpr int MD_DIM_MAX = 32;
constexpr unsigned int MD_SLICE_MIN = 256;  // references per work item at least (16 per wave of a 16-wave workgroup)
constexpr size_t MD_ITEMS_WANTED = 1024;    // as MB_ITEMS_WANTED

// the padded record width: the smallest of 4, 8, 16, 32 that is >= dim (dim in 1 .. 32)
inline int match_dims_padded(int dim) { return dim <= 4 ? 4 : dim <= 8 ? 8 : dim <= 16 ? 16 : 32; }
// references per work item at most
inline unsigned int match_dims_slice_max(int dp) { return dp <= 8 ? 2048u : dp == 16 ? 1024u : 512u; }

// MatchItem's layout (match_batch.hip): queries rec[q0 .. q0 + nq) against references rec[r0 .. r0 + nr), in RECORDS of DP
// floats; the references' indices in their own cloud are ridx0 ...; results for query q0 + i go to slot qslot0 + i
struct MatchDimsItem {
    uint32_t q0, nq, r0, nr, ridx0, qslot0, pad0, pad1;
};

// n records of `stride` bytes -> n records of dp floats at `out`.  Reads 4 * dim bytes of every record and no more (the last
// record of an array may end there).  Returns the number of valid records.
inline size_t match_dims_pack(const void* raw, size_t n, size_t stride, int dim, int dp, float* out) {
    const char* p = static_cast<const char*>(raw);
    size_t valid_n = 0;
    float v[MD_DIM_MAX];
    for (size_t i = 0; i < n; ++i, out += dp) {
        memcpy(v, p + i * stride, 4 * (size_t)dim);
        bool valid = true;
        for (int k = 0; k < dim; ++k) valid = valid && (v[k] - v[k]) == 0.0f;  // (finite: neither NaN nor +-inf)
        for (int k = 0; k < dp; ++k) out[k] = (valid && k < dim) ? v[k] : 0.0f;
        if (!valid) out[0] = std::numeric_limits<float>::infinity();
        valid_n += valid ? 1 : 0;
    }
    return valid_n;
}

struct MatchDimsPlan {
    struct Cloud { const void* p; size_t n, rec0; };
    std::vector<Cloud> clouds;      // every DISTINCT (pointer, length) of des1 once, in order of first appearance
    std::vector<size_t> cloud_of;   // per pair: its reference cloud
    std::vector<size_t> q_rec0;     // per pair: first record of its queries
    std::vector<size_t> q_slot0;    // n_pairs + 1: first result slot of its queries; [n_pairs] = all slots
    size_t n_rec = 0, n_slots = 0;  // records (references of distinct clouds, then queries); result slots (= queries)
    unsigned int slice = 0;         // references per item at most
    std::vector<MatchDimsItem> items;
};

struct MatchDimsPtrLenHash {
    size_t operator()(const std::pair<const void*, size_t>& k) const {
        return std::hash<const void*>()(k.first) ^ (std::hash<size_t>()(k.second) * 0x9e3779b97f4a7c15ull);
    }
};

// Lays the records out and builds the table.  false: more than 2^31 - 1 records or items (nothing usable in *plan).
inline bool match_dims_plan(size_t n_pairs, const void* const* des1, const size_t* n1, const size_t* n2, int dp, MatchDimsPlan* plan) {
    MatchDimsPlan& pl = *plan;
    pl.clouds.clear();
    pl.items.clear();
    pl.cloud_of.assign(n_pairs, 0);
    pl.q_rec0.assign(n_pairs, 0);
    pl.q_slot0.assign(n_pairs + 1, 0);
    pl.n_rec = pl.n_slots = 0;
    std::unordered_map<std::pair<const void*, size_t>, size_t, MatchDimsPtrLenHash> seen;
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
    for (size_t p = 0; p < n_pairs; ++p) {
        pl.q_rec0[p] = pl.n_rec;
        pl.q_slot0[p] = pl.n_slots;
        pl.n_rec += n2[p];
        pl.n_slots += n2[p];
    }
    pl.q_slot0[n_pairs] = pl.n_slots;
    if (pl.n_rec >= (1ull << 31)) return false;

    auto items_at = [&](unsigned int slice) {
        size_t c = 0;
        for (size_t p = 0; p < n_pairs; ++p)
            if (n2[p] && n1[p]) c += ((n2[p] + 63) / 64) * ((n1[p] + slice - 1) / slice);
        return c;
    };
    unsigned int slice = match_dims_slice_max(dp);
    while (slice > MD_SLICE_MIN && items_at(slice) < MD_ITEMS_WANTED) slice /= 2;
    pl.slice = slice;
    const size_t n_items = items_at(slice);
    if (n_items >= (1ull << 31)) return false;
    pl.items.reserve(n_items);
    // (the widest pairs first: their many slices start while the short items fill the gaps behind them)
    std::vector<size_t> order(n_pairs);
    for (size_t p = 0; p < n_pairs; ++p) order[p] = p;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return n1[a] > n1[b]; });
    for (size_t p : order) {
        if (!n2[p] || !n1[p]) continue;
        const MatchDimsPlan::Cloud& c = pl.clouds[pl.cloud_of[p]];
        for (size_t qb = 0; qb < n2[p]; qb += 64)
            for (size_t rb = 0; rb < c.n; rb += slice) {
                MatchDimsItem it;
                it.q0 = (uint32_t)(pl.q_rec0[p] + qb);
                it.nq = (uint32_t)std::min<size_t>(64, n2[p] - qb);
                it.r0 = (uint32_t)(c.rec0 + rb);
                it.nr = (uint32_t)std::min<size_t>(slice, c.n - rb);
                it.ridx0 = (uint32_t)rb;
                it.qslot0 = (uint32_t)(pl.q_slot0[p] + qb);
                it.pad0 = it.pad1 = 0;
                pl.items.push_back(it);
            }
    }
    return true;
}

}  // namespace pcc
