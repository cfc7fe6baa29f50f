// test_match_dims_plan.cpp -- csrc/match_dims_plan.hpp on the CPU (no library, no GPU): the padded record, invalid records,
// the bytes read of an array's last record, and the table of work items of pcc_match_knn_batch_dims.
//   1. packing: floats 0 .. dim-1 copied bit for bit, zeros behind them, (+inf, 0, ...) for a record with a non-finite float
//      among its first dim; a NaN at dim or beyond changes nothing
//   2. of every record 4 * dim bytes are read: the arrays here are heap blocks that END at the last record's 4 * dim bytes,
//      so that under AddressSanitizer (make asan) one byte more is an error
//   3. the table: every query of a pair in exactly one item per slice of its references, every reference of the pair in
//      exactly one slice, no item across a pair, shared reference clouds laid out once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <vector>
#include "match_dims_plan.hpp"

static int failures = 0;
#define REQUIRE(c)                                                                  \
    do {                                                                            \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++failures; } \
    } while (0)

static uint32_t bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

// n records of `stride` bytes in a block that ends after the last record's 4 * dim bytes; record i, float k = value(i, k)
static char* tight_array(size_t n, size_t stride, int dim, float (*value)(size_t, int)) {
    const size_t bytes = n ? (n - 1) * stride + 4 * (size_t)dim : 0;
    char* block = static_cast<char*>(std::malloc(bytes ? bytes : 1));
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (size_t i = 0; i < n; ++i)
        for (size_t k = 0; k < stride / 4; ++k) {
            if (i * stride + 4 * k + 4 > bytes) break;
            const float v = k < (size_t)dim ? value(i, (int)k) : nan;  // (the unread tail of a record holds NaN)
            std::memcpy(block + i * stride + 4 * k, &v, 4);
        }
    return block;
}

static float plain_value(size_t i, int k) { return (float)(i * 37 + k) * 0.25f - 3.0f; }
static float holed_value(size_t i, int k) {
    if (i == 1 && k == 0) return std::numeric_limits<float>::quiet_NaN();
    if (i == 3) return k == 0 ? std::numeric_limits<float>::infinity() : 1.0f;   // bin 0 ...
    return plain_value(i, k);
}
static int last_dim = 0;
static float last_bin_value(size_t i, int k) {  // ... and bin dim - 1
    if (i == 2 && k == last_dim - 1) return -std::numeric_limits<float>::infinity();
    if (i == 5 && k == last_dim - 1) return std::numeric_limits<float>::quiet_NaN();
    return plain_value(i, k);
}

static void test_pack() {
    const float inf = std::numeric_limits<float>::infinity();
    for (int dim = 1; dim <= 32; ++dim) {
        const int dp = pcc::match_dims_padded(dim);
        REQUIRE(dp >= dim && (dp == 4 || dp == 8 || dp == 16 || dp == 32) && (dp == 4 || dp / 2 < dim));
        for (size_t stride : {(size_t)4 * dim, (size_t)128, (size_t)256}) {
            const size_t n = 7;
            // every record valid: copied bit for bit, zero padded; NaN in the tail is never seen
            char* a = tight_array(n, stride, dim, plain_value);
            std::vector<float> out(n * dp, -1.f);
            REQUIRE(pcc::match_dims_pack(a, n, stride, dim, dp, out.data()) == n);
            for (size_t i = 0; i < n; ++i)
                for (int k = 0; k < dp; ++k) REQUIRE(bits(out[i * dp + k]) == bits(k < dim ? plain_value(i, k) : 0.0f));
            std::free(a);
            // non-finite floats in bin 0 and in bin dim - 1
            last_dim = dim;
            for (int which = 0; which < 2; ++which) {
                float (*value)(size_t, int) = which ? last_bin_value : holed_value;
                a = tight_array(n, stride, dim, value);
                const size_t valid = pcc::match_dims_pack(a, n, stride, dim, dp, out.data());
                size_t want_valid = 0;
                for (size_t i = 0; i < n; ++i) {
                    bool ok = true;
                    for (int k = 0; k < dim; ++k) ok = ok && std::isfinite(value(i, k));
                    want_valid += ok;
                    for (int k = 0; k < dp; ++k) {
                        const float want = !ok ? (k == 0 ? inf : 0.0f) : (k < dim ? value(i, k) : 0.0f);
                        REQUIRE(bits(out[i * dp + k]) == bits(want));
                    }
                }
                REQUIRE(valid == want_valid && valid == n - 2);
                std::free(a);
            }
        }
    }
    REQUIRE(pcc::match_dims_pack(nullptr, 0, 128, 32, 32, nullptr) == 0);
}

static void check_plan(const std::vector<size_t>& n1, const std::vector<size_t>& n2, const std::vector<int>& shares, int dp) {
    // des1 pointers: pair p shares the cloud of pair shares[p] (same pointer AND length), or has its own
    const size_t np = n1.size();
    static char arena[1 << 16];
    std::vector<const void*> des1(np);
    for (size_t p = 0; p < np; ++p) des1[p] = arena + (shares[p] >= 0 ? shares[p] : (int)p) * 64;
    pcc::MatchDimsPlan pl;
    REQUIRE(pcc::match_dims_plan(np, des1.data(), n1.data(), n2.data(), dp, &pl));
    REQUIRE(pl.slice >= pcc::MATCH_SLICE_MIN && pl.slice <= pcc::match_dims_slice_max(dp));
    size_t want_clouds = 0, want_rec = 0, want_slots = 0;
    for (size_t p = 0; p < np; ++p) {
        if (shares[p] < 0) { ++want_clouds; want_rec += n1[p]; }
        want_rec += n2[p];
        want_slots += n2[p];
    }
    REQUIRE(pl.clouds.size() == want_clouds && pl.n_rec == want_rec && pl.n_slots == want_slots && pl.q_slot0[np] == want_slots);
    // which pair a result slot / a record belongs to
    std::vector<int> pair_of_slot(pl.n_slots, -1), owner_of_rec(pl.n_rec, -1);  // owner: cloud c -> c, queries of pair p -> 1000000 + p
    for (size_t c = 0; c < pl.clouds.size(); ++c)
        for (size_t i = 0; i < pl.clouds[c].n; ++i) { REQUIRE(owner_of_rec[pl.clouds[c].rec0 + i] == -1); owner_of_rec[pl.clouds[c].rec0 + i] = (int)c; }
    for (size_t p = 0; p < np; ++p) {
        REQUIRE(pl.clouds[pl.cloud_of[p]].p == des1[p] && pl.clouds[pl.cloud_of[p]].n == n1[p]);
        for (size_t i = 0; i < n2[p]; ++i) {
            REQUIRE(owner_of_rec[pl.q_rec0[p] + i] == -1);
            owner_of_rec[pl.q_rec0[p] + i] = 1000000 + (int)p;
            pair_of_slot[pl.q_slot0[p] + i] = (int)p;
        }
    }
    for (int o : owner_of_rec) REQUIRE(o >= 0);  // the layout has no hole and no overlap
    // per (slot, reference index of the pair's cloud): how many items cover it
    std::vector<std::map<uint32_t, int> > slices_of_slot(pl.n_slots);  // slot -> ridx0 -> count
    for (const pcc::MatchItem& it : pl.items) {
        REQUIRE(it.nq >= 1 && it.nq <= 64 && it.nr >= 1 && it.nr <= pl.slice);
        const int p = pair_of_slot[it.qslot0];
        REQUIRE(p >= 0);
        const pcc::MatchDimsPlan::Cloud& c = pl.clouds[pl.cloud_of[p]];
        // no item across a pair: all its queries, slots and references are this pair's
        REQUIRE(it.q0 >= pl.q_rec0[p] && it.q0 + it.nq <= pl.q_rec0[p] + n2[p]);
        REQUIRE(it.qslot0 - pl.q_slot0[p] == it.q0 - pl.q_rec0[p] && (it.qslot0 - pl.q_slot0[p]) % 64 == 0);
        REQUIRE(it.r0 == c.rec0 + it.ridx0 && it.ridx0 % pl.slice == 0 && it.ridx0 + it.nr <= c.n);
        REQUIRE(it.nr == pl.slice || it.ridx0 + it.nr == c.n);
        REQUIRE(it.nq == 64 || it.q0 + it.nq == pl.q_rec0[p] + n2[p]);
        for (uint32_t i = 0; i < it.nq; ++i) ++slices_of_slot[it.qslot0 + i][it.ridx0];
    }
    size_t want_items = 0;
    for (size_t p = 0; p < np; ++p) {
        const size_t n_slices = n1[p] && n2[p] ? (n1[p] + pl.slice - 1) / pl.slice : 0;
        want_items += ((n2[p] + 63) / 64) * n_slices;
        for (size_t i = 0; i < n2[p]; ++i) {
            const std::map<uint32_t, int>& m = slices_of_slot[pl.q_slot0[p] + i];
            REQUIRE(m.size() == n_slices);  // every slice of the pair's references ...
            for (const auto& kv : m) REQUIRE(kv.second == 1 && kv.first < n1[p]);  // ... exactly once
        }
    }
    REQUIRE(pl.items.size() == want_items);
}

static void test_plan() {
    for (int dp : {4, 8, 16, 32}) {
        check_plan({1, 15, 16, 17, 255, 257, 2049, 0, 300, 2049}, {1, 63, 64, 65, 130, 1, 64, 5, 0, 129}, {-1, -1, -1, -1, -1, -1, -1, -1, -1, 6}, dp);
        check_plan({}, {}, {}, dp);
        check_plan({0}, {0}, {-1}, dp);
        // enough work that the slice stays at its maximum
        check_plan({23528, 23528, 5000}, {26308, 700, 4000}, {-1, 0, -1}, dp);
    }
    {  // the same pointer with ANOTHER length is another cloud
        static char arena[64];
        const void* des1[2] = {arena, arena};
        const size_t n1[2] = {5, 6}, n2[2] = {3, 3};
        pcc::MatchDimsPlan pl;
        REQUIRE(pcc::match_dims_plan(2, des1, n1, n2, 32, &pl) && pl.clouds.size() == 2 && pl.n_rec == 17);
    }
    {  // totals at 2^31 records are refused (nothing is allocated for them)
        static char arena[64];
        const void* des1[2] = {arena, arena + 4};
        const size_t n1[2] = {(size_t)1 << 30, (size_t)1 << 30}, n2[2] = {1, 1};
        pcc::MatchDimsPlan pl;
        REQUIRE(!pcc::match_dims_plan(2, des1, n1, n2, 4, &pl));
    }
}

int main() {
    test_pack();
    test_plan();
    if (failures) { std::printf("test_match_dims_plan: %d failure(s)\n", failures); return 1; }
    std::printf("test_match_dims_plan: ok\n");
    return 0;
}
